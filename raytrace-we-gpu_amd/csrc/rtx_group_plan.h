// rtx_group_plan.h — the partition and buffer arithmetic of a multi-GPU frame
// (include/rtx.h rtx_group): which rows each member renders, how large every
// buffer is, and the transfers that bring the members' rows to the root.
// No HIP in here: rtx_group.hip executes the plan on device memory, and
// tests/group_plan_check.cpp executes the same plan on host memory.
//
// A frame of `height` rows is cut into tiles of `tile_rows` rows; tile k
// belongs to member k % n (rtx_render_rows' partition). Member m
// renders its rows, ascending and contiguous, into its send buffer; member 0
// (the root) renders straight into slot 0 of the gathered buffer
// [n][max_rows][width]; one transfer per other member moves its rows to the
// start of slot m; rtx_deinterleave_rows turns the gathered buffer into the
// image [height][width].
// group_scatter_state / group_gather_state move a chain state between one
// whole frame and the members' parts (rtx_group_refine_import / _export),
// executed on host memory by tests/group_refine_check.cpp too.
// make_halo_plan lists the transfers of adaptive refinement's halo exchange
// (rtx_group_refine_adaptive), executed on host memory by
// tests/group_adaptive_check.cpp.
// The last part of the file is the frame split (rtx_group_accumulate):
// AccumPlan / accum_round, executed on host memory by
// tests/group_accum_check.cpp.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <vector>

namespace rtx {

constexpr size_t kGroupPixelBytes = 16;  // float4

// rtx_part_rows (rtx_api.hip) restated: rows of `part`.
inline uint32_t group_part_rows(uint32_t height, uint32_t tile_rows, uint32_t part, uint32_t nparts) {
    if (tile_rows == 0 || nparts == 0 || part >= nparts) return 0;
    const uint32_t tiles = (uint32_t)(((uint64_t)height + tile_rows - 1) / tile_rows);
    if (part >= tiles) return 0;
    const uint32_t my_tiles = (tiles - part + nparts - 1) / nparts;  // tiles part, part + nparts, ...
    uint64_t rows = (uint64_t)my_tiles * tile_rows;
    const uint32_t last_tile = part + (my_tiles - 1) * nparts;
    if (last_tile == tiles - 1) rows -= (uint64_t)tiles * tile_rows - height;  // ragged final tile
    return (uint32_t)rows;
}

// One transfer of the gather: `bytes` from offset 0 of member `member`'s send
// buffer to offset `dst_off` of the root's gathered buffer. A member without
// rows keeps its place with bytes == 0 (a copy skips it; a collective still
// names it).
struct GroupOp {
    uint32_t member;
    size_t dst_off;
    size_t bytes;
};

struct GroupPlan {
    uint32_t n = 0, width = 0, height = 0, tile_rows = 0;
    uint32_t max_rows = 0;             // rows of the largest part (part 0)
    std::vector<uint32_t> rows;        // [n] rows member m renders (0: it launches no render)
    std::vector<size_t> send_bytes;    // [n] member m's send buffer ([0]: 0, the root has none)
    size_t slot_bytes = 0;             // max_rows * width pixels
    size_t gathered_bytes = 0;         // n slots
    size_t image_bytes = 0;            // height * width pixels
    std::vector<GroupOp> ops;          // [n - 1] members 1 .. n-1, in order

    // Byte offset of member m's slot in the gathered buffer.
    size_t slot_off(uint32_t m) const { return (size_t)m * slot_bytes; }
    bool renders(uint32_t m) const { return rows[m] != 0; }
    bool same(uint32_t n_, uint32_t w, uint32_t h, uint32_t t) const {
        return n == n_ && width == w && height == h && tile_rows == t;
    }
};

// n >= 1, tile_rows >= 1, width * height <= 2^31 (rtx_set_frame's bound).
inline GroupPlan make_group_plan(uint32_t n, uint32_t width, uint32_t height, uint32_t tile_rows) {
    GroupPlan p;
    p.n = n;
    p.width = width;
    p.height = height;
    p.tile_rows = tile_rows;
    p.max_rows = group_part_rows(height, tile_rows, 0, n);
    const size_t row_bytes = (size_t)width * kGroupPixelBytes;
    p.slot_bytes = (size_t)p.max_rows * row_bytes;
    p.gathered_bytes = (size_t)n * p.slot_bytes;
    p.image_bytes = (size_t)height * row_bytes;
    p.rows.resize(n);
    p.send_bytes.assign(n, 0);
    for (uint32_t m = 0; m < n; ++m) {
        p.rows[m] = group_part_rows(height, tile_rows, m, n);
        if (m == 0) continue;
        p.send_bytes[m] = (size_t)p.rows[m] * row_bytes;
        p.ops.push_back(GroupOp{m, p.slot_off(m), p.send_bytes[m]});
    }
    return p;
}

// rtx_deinterleave_rows (rtx_kernels.hip k_deinterleave) restated: where image
// row y lives in the gathered buffer.
inline void group_row_owner(const GroupPlan &p, uint32_t y, uint32_t *member, uint32_t *local_row) {
    const uint32_t tile = y / p.tile_rows;
    *member = tile % p.n;
    *local_row = (tile / p.n) * p.tile_rows + (y - tile * p.tile_rows);
}

// ---- a chain state between one whole frame and the members' parts ----------
// (rtx_group_refine_export / rtx_group_refine_import, on host memory.) A
// member's chain state covers its own rows in its row order, group_row_owner's
// (member, local_row); the checkpoint is one whole-frame state
// [height][width] in framebuffer order. parts[m]: member m's rows[m] * width
// pixels of `pixel_bytes` each (ignored, and may be null, for a member without
// rows); whole: height * width pixels.
inline void group_scatter_state(const GroupPlan &p, const void *whole, void *const *parts,
                                size_t pixel_bytes = kGroupPixelBytes) {
    const size_t row_bytes = (size_t)p.width * pixel_bytes;
    for (uint32_t y = 0; y < p.height; ++y) {
        uint32_t m, r;
        group_row_owner(p, y, &m, &r);
        std::memcpy(static_cast<char *>(parts[m]) + (size_t)r * row_bytes,
                    static_cast<const char *>(whole) + (size_t)y * row_bytes, row_bytes);
    }
}
inline void group_gather_state(const GroupPlan &p, const void *const *parts, void *whole,
                               size_t pixel_bytes = kGroupPixelBytes) {
    const size_t row_bytes = (size_t)p.width * pixel_bytes;
    for (uint32_t y = 0; y < p.height; ++y) {
        uint32_t m, r;
        group_row_owner(p, y, &m, &r);
        std::memcpy(static_cast<char *>(whole) + (size_t)y * row_bytes,
                    static_cast<const char *>(parts[m]) + (size_t)r * row_bytes, row_bytes);
    }
}

// ---- the halo exchange of adaptive refinement (rtx_group_refine_adaptive) ---
// The activity rule reads a 3 x 3 window of err, which crosses tile edges
// (rtx_adaptive.h adaptive_active_rows). Every member packs its tiles' first
// and last err rows into an edge buffer [2][tiles][width] fp32 (plane 0: first
// rows, plane 1: last rows) and receives its halo buffer, same layout (plane
// 0: the row below each tile, plane 1: the row above). Tile k = m + j * n is
// member m's local tile j, so the row below it is the last row of member
// m - 1's local tile j (member n - 1's local tile j - 1 for m == 0) and the
// row above it the first row of member m + 1's local tile j (member 0's local
// tile j + 1 for m == n - 1): per member and direction one contiguous slab.
// A slot whose row lies outside the image is named by no transfer.
struct HaloOp {
    uint32_t src, dst;        // members: from src's edge buffer into dst's halo buffer
    size_t src_off, dst_off;  // bytes
    size_t bytes;
};

struct HaloPlan {
    uint32_t n = 0, width = 0, height = 0, tile_rows = 0;
    std::vector<uint32_t> tiles;  // [n] tiles of member m (0: it owns no rows)
    std::vector<HaloOp> ops;      // none for n == 1: the rule reads the local map

    // Bytes of member m's edge buffer, and of its halo buffer.
    size_t buffer_bytes(uint32_t m) const { return 2 * (size_t)tiles[m] * width * sizeof(float); }
    size_t slot_off(uint32_t m, uint32_t plane, uint32_t j) const {
        return ((size_t)plane * tiles[m] + j) * width * sizeof(float);
    }
    bool same(uint32_t n_, uint32_t w, uint32_t h, uint32_t t) const {
        return n == n_ && width == w && height == h && tile_rows == t;
    }
};

// n >= 1, tile_rows >= 1.
inline HaloPlan make_halo_plan(uint32_t n, uint32_t width, uint32_t height, uint32_t tile_rows) {
    HaloPlan p;
    p.n = n;
    p.width = width;
    p.height = height;
    p.tile_rows = tile_rows;
    const uint32_t tiles = (uint32_t)(((uint64_t)height + tile_rows - 1) / tile_rows);
    p.tiles.resize(n);
    for (uint32_t m = 0; m < n; ++m) p.tiles[m] = m >= tiles ? 0u : (tiles - m + n - 1) / n;
    if (n == 1) return p;
    const size_t row = (size_t)width * sizeof(float);
    for (uint32_t m = 0; m < n; ++m) {
        const uint32_t tm = p.tiles[m];
        if (tm == 0) continue;
        // below: the last rows (plane 1) of the member before
        if (m > 0)
            p.ops.push_back(HaloOp{m - 1, m, p.slot_off(m - 1, 1, 0), p.slot_off(m, 0, 0), tm * row});
        else if (tm > 1)  // (tile 0 has nothing below it)
            p.ops.push_back(HaloOp{n - 1, 0, p.slot_off(n - 1, 1, 0), p.slot_off(0, 0, 1), (tm - 1) * row});
        // above: the first rows (plane 0) of the member after, as far as its tiles go
        if (m + 1 < n) {
            if (p.tiles[m + 1] > 0)
                p.ops.push_back(HaloOp{m + 1, m, p.slot_off(m + 1, 0, 0), p.slot_off(m, 1, 0), p.tiles[m + 1] * row});
        } else {
            const uint32_t cnt = tm < p.tiles[0] - 1 ? tm : p.tiles[0] - 1;
            if (cnt > 0) p.ops.push_back(HaloOp{0, m, p.slot_off(0, 0, 1), p.slot_off(m, 1, 0), cnt * row});
        }
    }
    return p;
}

// ---- progressive frames dealt across the members (rtx_group_accumulate) ----
// The unit is a whole frame: with F frames accumulated, frame j of a call has
// frame_index F + j and goes to member j % n, so a call runs in rounds of up
// to n frames and always starts at member 0. In a round each taking member
// renders its frame's linear sums (rtx_render_sum) — the root into slot 0 of
// its sums buffer [n][pixels], member i > 0 into its own sum buffer [pixels] —
// one transfer per other taking member moves its sums to the start of slot i,
// and one rtx_fold_frames adds slots 0 .. m-1 (member order = frame order)
// into the accumulator [pixels] and writes the image [pixels].
struct AccumPlan {
    uint32_t n = 0, width = 0, height = 0;
    size_t pixels = 0;
    size_t slot_bytes = 0;   // one frame's sums: the accumulator, the image and a member's sum buffer too
    size_t sums_bytes = 0;   // the root's n slots

    size_t slot_off(uint32_t m) const { return (size_t)m * slot_bytes; }
    bool same(uint32_t n_, uint32_t w, uint32_t h) const { return n == n_ && width == w && height == h; }
};

// n >= 1, width * height <= 2^31 (rtx_set_frame's bound).
inline AccumPlan make_accum_plan(uint32_t n, uint32_t width, uint32_t height) {
    AccumPlan p;
    p.n = n;
    p.width = width;
    p.height = height;
    p.pixels = (size_t)width * height;
    p.slot_bytes = p.pixels * kGroupPixelBytes;
    p.sums_bytes = (size_t)n * p.slot_bytes;
    return p;
}

// A call of `frames` frames on top of F accumulated ones, spp samples per
// pixel and frame: the last frame_index fits the seed's 31 bits
// (0x80000000 | frame_index) and the final divisor (F + frames) * spp fits the
// fold kernel's uint32 (and is at least 1).
inline bool accum_call_valid(uint32_t F, uint32_t frames, uint32_t spp) {
    if (frames == 0 || spp == 0) return false;
    const uint64_t total = (uint64_t)F + frames;
    return total <= 0x7fffffffull && total * spp <= 0xffffffffull;
}

inline uint32_t accum_rounds(uint32_t n, uint32_t frames) { return frames / n + (frames % n ? 1u : 0u); }

// Round r (0 .. accum_rounds - 1) of such a call.
struct AccumRound {
    uint32_t m = 0;            // frames of the round: members 0 .. m-1 render, the others launch nothing
    uint32_t first_index = 0;  // member i < m renders frame_index first_index + i
    uint32_t frames_after = 0; // frames in the accumulator after the round's fold
    uint32_t divisor = 0;      // frames_after * spp
    std::vector<GroupOp> ops;  // [m - 1] members 1 .. m-1, in order: a whole slot each

    bool takes(uint32_t member) const { return member < m; }
    uint32_t frame_index(uint32_t member) const { return first_index + member; }
};

inline AccumRound accum_round(const AccumPlan &p, uint32_t F, uint32_t frames, uint32_t spp, uint32_t r) {
    AccumRound a;
    const uint64_t done = (uint64_t)r * p.n;  // frames of the call's earlier rounds
    const uint64_t left = frames - done;
    a.m = (uint32_t)(left < p.n ? left : p.n);
    a.first_index = (uint32_t)(F + done);
    a.frames_after = a.first_index + a.m;
    a.divisor = a.frames_after * spp;
    for (uint32_t i = 1; i < a.m; ++i) a.ops.push_back(GroupOp{i, p.slot_off(i), p.slot_bytes});
    return a;
}

}  // namespace rtx
