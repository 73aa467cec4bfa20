// group_refine_check — a chain state between one whole frame and the members'
// parts (raytrace-we-gpu_amd/csrc/rtx_group_plan.h group_scatter_state /
// group_gather_state), executed on host memory.
//
// rtx_group_refine_import scatters a whole-frame state [height][width] float4
// to the members (each its own rows, ascending and contiguous), and
// rtx_group_refine_export gathers them back. Here a "pixel" is a (y, x) tag
// with special float bit patterns beside it; the part buffers sit between
// guard words. After a scatter every part's rows must be the rows the
// partition gives it by definition (tile k belongs to member k % n: Python's
// part_row_ids), in ascending order; the gather of the scatter must be the
// whole, bit for bit; and no guard word may change.
//
//   group_refine_check            -> one JSON line; exit 1 on any mismatch
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_group_plan.h"

namespace {

struct Px {  // one 16-byte pixel of a chain state
    uint32_t y, x, bits, magic;
};
static_assert(sizeof(Px) == rtx::kGroupPixelBytes, "a pixel is a float4");
constexpr uint32_t kMagic = 0x52465243u, kGuard = 0xA5A5A5A5u;
constexpr size_t kGuardPx = 4;  // guard pixels on either side of a part
// NaN, -0, a denormal, +inf: a state's bits travel untouched
constexpr uint32_t kSpecial[4] = {0x7fc00001u, 0x80000000u, 0x00000001u, 0x7f800000u};

struct Counts {
    unsigned long long cases = 0, rows_checked = 0, mismatches = 0, guard_hits = 0, idle_members = 0;
};

void check_case(uint32_t W, uint32_t H, uint32_t T, uint32_t n, Counts &c) {
    c.cases++;
    const rtx::GroupPlan p = rtx::make_group_plan(n, W, H, T);
    std::vector<Px> whole((size_t)W * H);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) whole[(size_t)y * W + x] = Px{y, x, kSpecial[(y * W + x) % 4], kMagic};

    // the parts, each between guards
    std::vector<std::vector<Px>> store(n);
    std::vector<void *> parts(n, nullptr);
    std::vector<const void *> cparts(n, nullptr);
    for (uint32_t m = 0; m < n; ++m) {
        store[m].assign((size_t)p.rows[m] * W + 2 * kGuardPx, Px{kGuard, kGuard, kGuard, kGuard});
        if (p.rows[m] == 0) {
            c.idle_members++;
            continue;  // a member without rows takes no buffer
        }
        parts[m] = store[m].data() + kGuardPx;
        cparts[m] = parts[m];
    }
    rtx::group_scatter_state(p, whole.data(), parts.data());

    // every part's rows: the rows of the partition's definition, ascending
    for (uint32_t m = 0; m < n; ++m) {
        uint32_t r = 0;
        for (uint32_t y = 0; y < H; ++y) {
            if ((y / T) % n != m) continue;
            if (r >= p.rows[m]) {
                c.mismatches++;
                break;
            }
            const Px *row = store[m].data() + kGuardPx + (size_t)r * W;
            if (std::memcmp(row, &whole[(size_t)y * W], (size_t)W * sizeof(Px)) != 0) c.mismatches++;
            c.rows_checked++;
            ++r;
        }
        if (r != p.rows[m]) c.mismatches++;
        for (size_t g = 0; g < kGuardPx; ++g) {
            if (store[m][g].magic != kGuard || store[m][store[m].size() - 1 - g].magic != kGuard) c.guard_hits++;
        }
    }

    // the gather of the scatter is the identity
    std::vector<Px> back((size_t)W * H + 2 * kGuardPx, Px{kGuard, kGuard, kGuard, kGuard});
    rtx::group_gather_state(p, cparts.data(), back.data() + kGuardPx);
    if (std::memcmp(back.data() + kGuardPx, whole.data(), whole.size() * sizeof(Px)) != 0) c.mismatches++;
    for (size_t g = 0; g < kGuardPx; ++g)
        if (back[g].magic != kGuard || back[back.size() - 1 - g].magic != kGuard) c.guard_hits++;
}

}  // namespace

int main() {
    Counts c;
    // (W, H, T, n): a ragged last tile and a member without rows; odd sizes;
    // one row for two members; one member
    const uint32_t cases[][4] = {{7, 20, 8, 4}, {5, 9, 2, 3}, {3, 1, 1, 2}, {4, 6, 3, 1}};
    for (const auto &k : cases) check_case(k[0], k[1], k[2], k[3], c);
    std::printf("{\"cases\": %llu, \"rows_checked\": %llu, \"mismatches\": %llu, \"guard_hits\": %llu, "
                "\"idle_members\": %llu}\n",
                c.cases, c.rows_checked, c.mismatches, c.guard_hits, c.idle_members);
    return c.mismatches == 0 && c.guard_hits == 0 ? 0 : 1;
}
