// group_accum_check — the plan of progressive frames dealt across a group's
// members (raytrace-we-gpu_amd/csrc/rtx_group_plan.h: AccumPlan, accum_round),
// executed on host memory.
//
// rtx_group.hip executes the plan with device buffers: in every round each
// taking member renders its frame's sums (the root into slot 0 of its sums
// buffer, the others into their own sum buffer), one transfer per other taking
// member moves them into its slot, and the fold adds the round's slots in
// order into the accumulator and writes the image. Here a member's "render"
// writes a tag that depends on (frame_index, pixel), the transfers are memcpy,
// and the fold is the kernel's loop in fp32 (the image without its gamma:
// accumulator / divisor). The result must equal a plain sequential
// one-accumulator emulation exactly, no access may leave its buffer, no member
// may render beyond the call's frames, and every frame_index must be used
// exactly once. The tags are order-sensitive (1e8, 1 and -1e8, mixed): the
// checker folds every round of three or more slots once more in reverse slot
// order and requires a changed pixel, so a reordered fold could not pass.
//
//   group_accum_check           -> one JSON line; exit 1 on any failure
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_group_plan.h"

namespace {

struct Px {  // one 16-byte pixel
    float x, y, z, w;
};
static_assert(sizeof(Px) == rtx::kGroupPixelBytes, "a pixel is a float4");

struct Counts {
    unsigned long long frames_rendered = 0, rounds = 0, ops = 0, mismatches = 0, out_of_bounds = 0, idle_renders = 0,
                       order_rounds = 0, order_blind = 0;
};

// A buffer that refuses accesses outside itself.
struct Buf {
    std::vector<unsigned char> bytes;
    bool in(size_t off, size_t n) const { return off <= bytes.size() && n <= bytes.size() - off; }
    bool get(size_t off, Px *p) const {
        if (!in(off, sizeof(Px))) return false;
        std::memcpy(p, bytes.data() + off, sizeof(Px));
        return true;
    }
    bool put(size_t off, const Px &p) {
        if (!in(off, sizeof(Px))) return false;
        std::memcpy(bytes.data() + off, &p, sizeof(Px));
        return true;
    }
};

// What member "renders" for (frame_index, pixel): x is order-sensitive in fp32
// ((1e8 + 1) - 1e8 = 0 but (1e8 - 1e8) + 1 = 1), y and z are small integers
// whose sums are exact and tell a missing, doubled or swapped frame.
Px tag(uint32_t frame_index, uint32_t pixel) {
    static const float rot[3] = {1e8f, 1.0f, -1e8f};
    Px t;
    // (hashed, not a plain rotation: a periodic sequence can read the same backwards)
    t.x = rot[((((frame_index + 1) * 2654435761u) ^ ((pixel + 1) * 40503u)) >> 13) % 3];
    t.y = (float)((frame_index + 1) * (pixel + 1));
    t.z = (float)((frame_index + 1) * (frame_index + 1));
    t.w = 0.0f;
    return t;
}

struct Call {
    uint32_t frames;
    bool reset;
};

// The kernel's loop: accum[p].xyz += sums[k * slot_pixels + p].xyz, k = 0 .. m-1
// (reverse: the same slots last to first), image[p] = accum[p] / divisor.
void fold(Buf &accum, const Buf &sums, uint32_t m, size_t slot_pixels, size_t pixels, uint32_t divisor, Buf &image,
          bool reverse, Counts &c) {
    const float n = (float)divisor;
    for (size_t p = 0; p < pixels; ++p) {
        Px a;
        if (!accum.get(p * sizeof(Px), &a)) {
            c.out_of_bounds++;
            continue;
        }
        for (uint32_t kk = 0; kk < m; ++kk) {
            const uint32_t k = reverse ? m - 1 - kk : kk;
            Px s;
            if (!sums.get(((size_t)k * slot_pixels + p) * sizeof(Px), &s)) {
                c.out_of_bounds++;
                continue;
            }
            a.x = a.x + s.x;
            a.y = a.y + s.y;
            a.z = a.z + s.z;
        }
        const Px o{a.x / n, a.y / n, a.z / n, 1.0f};
        if (!accum.put(p * sizeof(Px), a) || !image.put(p * sizeof(Px), o)) c.out_of_bounds++;
    }
}

void check_case(uint32_t n, const std::vector<Call> &calls, uint32_t W, uint32_t H, uint32_t spp, Counts &c) {
    const rtx::AccumPlan plan = rtx::make_accum_plan(n, W, H);
    const size_t pixels = (size_t)W * H;
    if (plan.pixels != pixels || plan.slot_bytes != pixels * sizeof(Px) || plan.sums_bytes != n * plan.slot_bytes)
        c.mismatches++;
    Buf accum, sums, image, ref, ref_image;
    accum.bytes.assign(plan.slot_bytes, 0);
    image.bytes.assign(plan.slot_bytes, 0);
    sums.bytes.assign(plan.sums_bytes, 0);
    ref.bytes.assign(pixels * sizeof(Px), 0);
    ref_image.bytes.assign(pixels * sizeof(Px), 0);
    std::vector<Buf> send(n);
    for (uint32_t i = 1; i < n; ++i) send[i].bytes.assign(plan.slot_bytes, 0);

    uint32_t F = 0;              // frames accumulated (the group's state)
    std::vector<uint32_t> used;  // renders per frame_index since the last restart
    bool order_seen = false, need_order = false;
    for (const Call &call : calls) {
        if (call.reset || F == 0) {  // restart: zeroed accumulator, frame_index from 0
            F = 0;
            std::fill(accum.bytes.begin(), accum.bytes.end(), 0);
            std::fill(ref.bytes.begin(), ref.bytes.end(), 0);
            used.clear();
        }
        if (!rtx::accum_call_valid(F, call.frames, spp)) {
            c.mismatches++;
            continue;
        }
        used.resize((size_t)F + call.frames, 0);
        const uint32_t rounds = rtx::accum_rounds(n, call.frames);
        if (rounds != (call.frames + n - 1) / n) c.mismatches++;
        uint32_t done = 0;  // frames of the call folded so far
        for (uint32_t r = 0; r < rounds; ++r) {
            const rtx::AccumRound round = rtx::accum_round(plan, F, call.frames, spp, r);
            c.rounds++;
            // the renders: by definition frame j of the call goes to member j % n
            uint32_t takers = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const uint64_t j = (uint64_t)r * n + i;
                const bool owns = j < call.frames;
                if (round.takes(i) && !owns) c.idle_renders++;  // a render beyond the call's frames
                if (!round.takes(i) && owns) c.mismatches++;     // a frame nobody renders
                if (!round.takes(i)) continue;
                takers++;
                const uint32_t fi = round.frame_index(i);
                if (owns && fi != F + j) c.mismatches++;
                if (fi < used.size()) used[fi]++;
                else c.out_of_bounds++;
                c.frames_rendered++;
                Buf &dst = i == 0 ? sums : send[i];
                const size_t base = i == 0 ? plan.slot_off(0) : 0;
                for (uint32_t p = 0; p < pixels; ++p)
                    if (!dst.put(base + (size_t)p * sizeof(Px), tag(fi, p))) c.out_of_bounds++;
            }
            if (takers != round.m || round.m == 0 || round.m > n) c.mismatches++;
            if (round.ops.size() != round.m - 1) c.mismatches++;
            // the gather
            uint32_t expect_member = 1;
            for (const rtx::GroupOp &op : round.ops) {
                c.ops++;
                if (op.member != expect_member++ || op.member >= round.m) {
                    c.mismatches++;
                    continue;
                }
                if (op.bytes != plan.slot_bytes || op.dst_off != plan.slot_off(op.member)) c.mismatches++;
                if (!send[op.member].in(0, op.bytes) || !sums.in(op.dst_off, op.bytes)) {
                    c.out_of_bounds++;
                    continue;
                }
                std::memcpy(sums.bytes.data() + op.dst_off, send[op.member].bytes.data(), op.bytes);
            }
            // the divisor, by the definition: (frames accumulated after the round) * spp
            done += round.m;
            if (round.frames_after != F + done || round.divisor != (F + done) * spp) c.mismatches++;
            // order sensitivity of this round's data: the same slots in reverse
            if (round.m >= 3) {
                Buf acc_rev = accum, img_rev = image;
                Buf acc_fwd = accum, img_fwd = image;
                fold(acc_fwd, sums, round.m, pixels, pixels, round.divisor, img_fwd, false, c);
                fold(acc_rev, sums, round.m, pixels, pixels, round.divisor, img_rev, true, c);
                c.order_rounds++;
                need_order = true;
                if (acc_rev.bytes == acc_fwd.bytes) c.order_blind++;
                else order_seen = true;
            }
            fold(accum, sums, round.m, pixels, pixels, round.divisor, image, false, c);
        }
        // the sequential emulation: one accumulator, the call's frames in order
        for (uint32_t j = 0; j < call.frames; ++j)
            for (uint32_t p = 0; p < pixels; ++p) {
                Px a{};
                ref.get((size_t)p * sizeof(Px), &a);
                const Px s = tag(F + j, p);
                a.x = a.x + s.x;
                a.y = a.y + s.y;
                a.z = a.z + s.z;
                ref.put((size_t)p * sizeof(Px), a);
                const float nn = (float)((F + j + 1) * spp);
                ref_image.put((size_t)p * sizeof(Px), Px{a.x / nn, a.y / nn, a.z / nn, 1.0f});
            }
        F += call.frames;
        if (accum.bytes != ref.bytes || image.bytes != ref_image.bytes) c.mismatches++;
        for (uint32_t u : used)
            if (u != 1) c.mismatches++;  // every frame_index exactly once
    }
    if (need_order && !order_seen) c.mismatches++;  // a case whose tags could not see a reordered fold
}

}  // namespace

int main() {
    Counts c;
    unsigned ncases = 0;
    const struct {
        uint32_t n;
        std::vector<Call> calls;
    } cases[] = {
        {3, {{7, false}, {2, false}}}, {4, {{2, false}}},          {1, {{3, false}}},
        {8, {{8, false}, {8, false}}}, {5, {{1, false}, {1, false}, {1, false}}}, {64, {{65, false}}},
        {3, {{4, false}, {5, true}}},  // a reset between the calls
    };
    for (const auto &k : cases) {
        check_case(k.n, k.calls, 37, 1, 3, c);
        ++ncases;
    }
    // the call's bounds (frame_index within 31 bits, divisor within uint32)
    const struct {
        uint32_t F, frames, spp;
        bool ok;
    } bounds[] = {{0, 0, 1, false},           {0, 1, 0, false},          {0x7ffffffeu, 1, 1, true},
                  {0x7ffffffeu, 2, 1, false}, {0, 0x10000u, 0x10000u, false}, {0, 0xffffu, 0x10001u, true},
                  {0xffffffffu, 1, 1, false}, {5, 0xffffffffu, 1, false}};
    for (const auto &b : bounds)
        if (rtx::accum_call_valid(b.F, b.frames, b.spp) != b.ok) c.mismatches++;
    const bool order_sensitive = c.order_rounds > 0 && c.order_blind == 0;
    std::printf("{\"cases\": %u, \"frames_rendered\": %llu, \"rounds\": %llu, \"ops\": %llu, \"idle_renders\": %llu, "
                "\"out_of_bounds\": %llu, \"mismatches\": %llu, \"order_rounds\": %llu, \"order_sensitive\": %s}\n",
                ncases, c.frames_rendered, c.rounds, c.ops, c.idle_renders, c.out_of_bounds, c.mismatches,
                c.order_rounds, order_sensitive ? "true" : "false");
    return (c.mismatches || c.out_of_bounds || c.idle_renders || !order_sensitive) ? 1 : 0;
}
