// group_adaptive_check — the activity rule of adaptive refinement on row parts
// (raytrace-we-gpu_amd/csrc/rtx_adaptive.h adaptive_active_rows) and the halo
// exchange that feeds it (rtx_group_plan.h make_halo_plan), executed on host
// memory.
//
// For every (H, T, n) with H in 1..13, T in 1..5, n in 1..5 and widths 1, 2
// and 7: random whole-frame maps (err with NaN, +-inf and values equal to the
// threshold; counts against a cap) are scattered to the parts; every part's
// edge buffer is built from the whole frame by the layout's definition (plane
// 0: each tile's first err row, plane 1: its last); the halo plan's transfers
// run between guard words; then adaptive_active_rows is evaluated for every
// local pixel of every part. The union must be adaptive_active on the whole
// frame, pixel for pixel. A halo slot that stands for a row outside the image
// must not be written by the plan (it keeps a tagged NaN) and must not be read
// by the rule (for the evaluation it holds +inf, which would switch its
// neighbours on). A uniform state (every err +inf) must give the same answer
// with no halo at all.
//
//   group_adaptive_check          -> one JSON line; exit 1 on any mismatch
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_adaptive.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_group_plan.h"

namespace {

constexpr uint32_t kGuard = 0xA5A5A5A5u, kUnset = 0x7fc0deadu;  // (a NaN no err value carries)
constexpr size_t kGuardWords = 4;

struct Counts {
    unsigned long long cases = 0, pixels = 0, active = 0, halo_only = 0, transfers = 0, mismatches = 0, guard_hits = 0,
                       outside_written = 0, unfilled = 0, idle_members = 0;
};

uint32_t rng_state = 0x2545F491u;
uint32_t rnd() {  // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

uint32_t float_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

// A buffer of `words` 32-bit words between guards.
struct Guarded {
    std::vector<uint32_t> w;
    explicit Guarded(size_t words, uint32_t fill) : w(words + 2 * kGuardWords, fill) {
        for (size_t g = 0; g < kGuardWords; ++g) w[g] = w[w.size() - 1 - g] = kGuard;
    }
    uint32_t *data() { return w.data() + kGuardWords; }
    bool intact() const {
        for (size_t g = 0; g < kGuardWords; ++g)
            if (w[g] != kGuard || w[w.size() - 1 - g] != kGuard) return false;
        return true;
    }
};

void check_case(uint32_t W, uint32_t H, uint32_t T, uint32_t n, Counts &c) {
    c.cases++;
    const float thr_choice[3] = {0.5f, INFINITY, 0.0f};
    const uint32_t cap_choice[3] = {0u, 24u, 8u};
    const float thr = thr_choice[c.cases % 3];
    const uint32_t samples = 8u, cap = cap_choice[(c.cases / 3) % 3];
    const size_t px = (size_t)W * H;
    std::vector<float> err(px);
    std::vector<uint32_t> count(px);
    for (size_t i = 0; i < px; ++i) {
        switch (rnd() % 12) {
            case 0: err[i] = NAN; break;
            case 1: err[i] = INFINITY; break;
            case 2: err[i] = -INFINITY; break;
            case 3: err[i] = thr; break;  // equal to the threshold: active
            case 4: err[i] = 0.75f; break;
            default: err[i] = 0.25f * (float)(rnd() % 1000) / 1000.0f; break;  // mostly quiet: the edges matter
        }
        count[i] = rnd() % 33;
    }
    const rtx::GroupPlan gp = rtx::make_group_plan(n, W, H, T);
    const rtx::HaloPlan hp = rtx::make_halo_plan(n, W, H, T);
    const uint32_t tiles = (H + T - 1) / T;

    // the parts' maps (group_scatter_state at 4 bytes a pixel)
    std::vector<std::vector<float>> perr(n);
    std::vector<std::vector<uint32_t>> pcount(n);
    std::vector<void *> pe(n, nullptr), pc(n, nullptr);
    for (uint32_t m = 0; m < n; ++m) {
        perr[m].resize((size_t)gp.rows[m] * W);
        pcount[m].resize((size_t)gp.rows[m] * W);
        pe[m] = perr[m].data();
        pc[m] = pcount[m].data();
        if (gp.rows[m] == 0) c.idle_members++;
        if (hp.tiles[m] != rtx::adaptive_part_tiles(H, T, m, n)) c.mismatches++;
        if ((gp.rows[m] == 0) != (hp.tiles[m] == 0)) c.mismatches++;
    }
    rtx::group_scatter_state(gp, err.data(), pe.data(), sizeof(float));
    rtx::group_scatter_state(gp, count.data(), pc.data(), sizeof(uint32_t));

    // edges by definition, from the whole frame; halos unset
    std::vector<Guarded> edges, halo;
    for (uint32_t m = 0; m < n; ++m) {
        const size_t words = hp.buffer_bytes(m) / sizeof(uint32_t);
        edges.emplace_back(words, kUnset);
        halo.emplace_back(words, kUnset);
        for (uint32_t j = 0; j < hp.tiles[m]; ++j) {
            const uint32_t k = m + j * n, first = k * T, last = (first + T < H ? first + T : H) - 1;
            std::memcpy(edges[m].data() + hp.slot_off(m, 0, j) / 4, &err[(size_t)first * W], W * sizeof(float));
            std::memcpy(edges[m].data() + hp.slot_off(m, 1, j) / 4, &err[(size_t)last * W], W * sizeof(float));
        }
    }
    if (n == 1 && !hp.ops.empty()) c.mismatches++;
    for (const rtx::HaloOp &op : hp.ops) {
        c.transfers++;
        if (op.src >= n || op.dst >= n || op.src == op.dst || op.bytes == 0 || op.bytes % (W * sizeof(float)) != 0 ||
            op.src_off + op.bytes > hp.buffer_bytes(op.src) || op.dst_off + op.bytes > hp.buffer_bytes(op.dst)) {
            c.mismatches++;
            continue;
        }
        std::memcpy(reinterpret_cast<char *>(halo[op.dst].data()) + op.dst_off,
                    reinterpret_cast<const char *>(edges[op.src].data()) + op.src_off, op.bytes);
    }
    // at most two slabs per direction between a pair of members
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            unsigned cnt = 0;
            for (const rtx::HaloOp &op : hp.ops) cnt += op.src == a && op.dst == b;
            if (cnt > 2) c.mismatches++;
        }
    // every slot inside the image is filled with its row, every slot outside it untouched
    for (uint32_t m = 0; m < n; ++m) {
        if (!edges[m].intact() || !halo[m].intact()) c.guard_hits++;
        for (uint32_t j = 0; n > 1 && j < hp.tiles[m]; ++j) {
            const uint32_t k = m + j * n;
            for (uint32_t plane = 0; plane < 2; ++plane) {
                uint32_t *slot = halo[m].data() + hp.slot_off(m, plane, j) / 4;
                const bool outside = plane == 0 ? k == 0 : k == tiles - 1;
                for (uint32_t x = 0; x < W; ++x) {
                    if (outside) {
                        if (slot[x] != kUnset) c.outside_written++;
                        slot[x] = float_bits(INFINITY);  // a read would switch the neighbours on
                    } else {
                        const uint32_t y = plane == 0 ? k * T - 1 : (k + 1) * T;
                        if (slot[x] != float_bits(err[(size_t)y * W + x])) c.unfilled++;
                    }
                }
            }
        }
    }

    // the rule on every part against the rule on the whole frame
    for (uint32_t y = 0; y < H; ++y) {
        uint32_t m, lr;
        rtx::group_row_owner(gp, y, &m, &lr);
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t gi = y * W + x, li = lr * W + x;
            const bool want = rtx::adaptive_active(err.data(), count.data(), gi, W, H, samples, thr, cap);
            const float *h = n == 1 ? nullptr : reinterpret_cast<const float *>(halo[m].data());
            const bool got = rtx::adaptive_active_rows(perr[m].data(), pcount[m].data(), h, li, W, H, T, m, n, samples,
                                                       thr, cap);
            c.pixels++;
            c.active += want;
            if (got != want) c.mismatches++;
            // (how many answers hang on the halo: active, but not by the part's own rows)
            if (want && n > 1 &&
                !rtx::adaptive_active_rows(perr[m].data(), pcount[m].data(), nullptr, li, W, H, T, m, n, samples, thr, cap))
                c.halo_only++;
        }
    }

    // a uniform state needs no halo
    std::vector<float> inf(px, INFINITY);
    for (uint32_t y = 0; y < H; ++y) {
        uint32_t m, lr;
        rtx::group_row_owner(gp, y, &m, &lr);
        for (uint32_t x = 0; x < W; ++x) {
            const bool want = rtx::adaptive_active(inf.data(), count.data(), y * W + x, W, H, samples, thr, cap);
            const bool got = rtx::adaptive_active_rows(inf.data(), pcount[m].data(), nullptr, lr * W + x, W, H, T, m, n,
                                                       samples, thr, cap);
            if (got != want) c.mismatches++;
        }
    }
}

}  // namespace

int main() {
    Counts c;
    const uint32_t widths[3] = {1, 2, 7};
    for (uint32_t H = 1; H <= 13; ++H)
        for (uint32_t T = 1; T <= 5; ++T)
            for (uint32_t n = 1; n <= 5; ++n)
                for (uint32_t W : widths) check_case(W, H, T, n, c);
    std::printf("{\"cases\": %llu, \"pixels\": %llu, \"active\": %llu, \"halo_only\": %llu, \"transfers\": %llu, "
                "\"mismatches\": %llu, \"guard_hits\": %llu, \"outside_written\": %llu, \"unfilled\": %llu, "
                "\"idle_members\": %llu}\n",
                c.cases, c.pixels, c.active, c.halo_only, c.transfers, c.mismatches, c.guard_hits, c.outside_written,
                c.unfilled, c.idle_members);
    return c.mismatches == 0 && c.guard_hits == 0 && c.outside_written == 0 && c.unfilled == 0 ? 0 : 1;
}
