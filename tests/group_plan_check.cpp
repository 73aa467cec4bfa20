// group_plan_check — the multi-GPU frame's plan (raytrace-we-gpu_amd/csrc/
// rtx_group_plan.h), executed on host memory.
//
// rtx_group.hip executes the plan with device buffers: every member renders
// its rows into its send buffer (the root into slot 0 of the gathered buffer),
// one transfer per other member moves them into its slot, and the
// de-interleave builds the image. Here a "pixel" is a (member, local row) tag,
// the render fills a member's buffer with its tags, the transfers are memcpy,
// and the de-interleave is the kernel's index arithmetic restated. Every
// image row must then carry the tag of the member and local row that own it
// (by the partition's definition: tile k belongs to member k % n), no access
// may leave its buffer, and a member without rows must not render.
//
//   group_plan_check            -> one JSON line; exit 1 on any mismatch
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_group_plan.h"

namespace {

struct Tag {  // one 16-byte pixel
    uint32_t member, local_row, x, magic;
};
static_assert(sizeof(Tag) == rtx::kGroupPixelBytes, "a pixel is a float4");
constexpr uint32_t kMagic = 0x52545847u;

struct Counts {
    unsigned long long rows_checked = 0, mismatches = 0, out_of_bounds = 0, idle_renders = 0, ops = 0, idle_members = 0;
};

// A buffer that refuses accesses outside itself.
struct Buf {
    std::vector<unsigned char> bytes;
    bool in(size_t off, size_t n) const { return off <= bytes.size() && n <= bytes.size() - off; }
};

void check_case(uint32_t H, uint32_t T, uint32_t n, uint32_t W, Counts &c) {
    const rtx::GroupPlan p = rtx::make_group_plan(n, W, H, T);
    Buf gathered, image;
    gathered.bytes.assign(p.gathered_bytes, 0);
    image.bytes.assign(p.image_bytes, 0);
    std::vector<Buf> send(n);
    for (uint32_t m = 1; m < n; ++m) send[m].bytes.assign(p.send_bytes[m], 0);
    const size_t row_bytes = (size_t)W * sizeof(Tag);

    // the plan's own sums
    unsigned long long total_rows = 0;
    for (uint32_t m = 0; m < n; ++m) {
        total_rows += p.rows[m];
        if (p.rows[m] > p.max_rows) c.mismatches++;
    }
    if (total_rows != H) c.mismatches++;
    if (p.ops.size() != n - 1) c.mismatches++;

    // rows each member owns by the partition's definition (tile k -> member k % n)
    std::vector<uint32_t> own(n, 0);
    for (uint32_t y = 0; y < H; ++y) own[(y / T) % n]++;

    // "render": member m writes rows[m] rows of tags at the start of its buffer
    for (uint32_t m = 0; m < n; ++m) {
        if (own[m] == 0) c.idle_members++;
        if (p.renders(m) && own[m] == 0) c.idle_renders++;  // a render launched for no rows
        if (!p.renders(m) && own[m] != 0) c.mismatches++;   // rows nobody renders
        if (!p.renders(m)) continue;
        Buf &dst = m == 0 ? gathered : send[m];
        const size_t base = m == 0 ? p.slot_off(0) : 0;
        for (uint32_t r = 0; r < p.rows[m]; ++r)
            for (uint32_t x = 0; x < W; ++x) {
                const size_t off = base + (size_t)r * row_bytes + (size_t)x * sizeof(Tag);
                if (!dst.in(off, sizeof(Tag))) {
                    c.out_of_bounds++;
                    continue;
                }
                const Tag t{m, r, x, kMagic};
                std::memcpy(dst.bytes.data() + off, &t, sizeof t);
            }
    }

    // the gather's transfers
    for (const rtx::GroupOp &op : p.ops) {
        c.ops++;
        if (op.member == 0 || op.member >= n) {
            c.mismatches++;
            continue;
        }
        if (op.bytes != p.send_bytes[op.member] || op.bytes != (size_t)p.rows[op.member] * row_bytes) c.mismatches++;
        if (op.dst_off != p.slot_off(op.member) || op.bytes > p.slot_bytes) c.mismatches++;
        if (!send[op.member].in(0, op.bytes) || !gathered.in(op.dst_off, op.bytes)) {
            c.out_of_bounds++;
            continue;
        }
        if (op.bytes) std::memcpy(gathered.bytes.data() + op.dst_off, send[op.member].bytes.data(), op.bytes);
    }

    // the de-interleave (k_deinterleave's index arithmetic): image pixel (y, x)
    // = gathered[(part * max_rows + local_row) * width + x]
    for (uint32_t y = 0; y < H; ++y) {
        uint32_t part, lr;
        rtx::group_row_owner(p, y, &part, &lr);
        const size_t src = ((size_t)part * p.max_rows + lr) * row_bytes;
        const size_t dst = (size_t)y * row_bytes;
        if (!gathered.in(src, row_bytes) || !image.in(dst, row_bytes)) {
            c.out_of_bounds++;
            continue;
        }
        std::memcpy(image.bytes.data() + dst, gathered.bytes.data() + src, row_bytes);
    }

    // every image row holds the tags of its owner, by the partition's
    // definition and independent of the plan: tile k -> member k % n, and the
    // local row counts the member's earlier rows
    std::vector<uint32_t> seen(n, 0);
    for (uint32_t y = 0; y < H; ++y) {
        const uint32_t owner = (y / T) % n;
        const uint32_t local = seen[owner]++;
        c.rows_checked++;
        for (uint32_t x = 0; x < W; ++x) {
            Tag t;
            std::memcpy(&t, image.bytes.data() + (size_t)y * row_bytes + (size_t)x * sizeof(Tag), sizeof t);
            if (t.member != owner || t.local_row != local || t.x != x || t.magic != kMagic) {
                c.mismatches++;
                break;
            }
        }
    }
    for (uint32_t m = 0; m < n; ++m)
        if (seen[m] != p.rows[m]) c.mismatches++;
}

}  // namespace

int main() {
    const uint32_t cases[][3] = {{1080, 5, 8}, {1081, 5, 8}, {117, 8, 3}, {117, 64, 5},
                                 {10, 3, 8},   {1, 1, 2},    {20, 8, 4}};
    Counts c;
    unsigned ncases = 0;
    for (const auto &k : cases) {
        check_case(k[0], k[1], k[2], 7, c);
        ++ncases;
    }
    std::printf("{\"cases\": %u, \"rows_checked\": %llu, \"ops\": %llu, \"idle_members\": %llu, "
                "\"idle_renders\": %llu, \"out_of_bounds\": %llu, \"mismatches\": %llu}\n",
                ncases, c.rows_checked, c.ops, c.idle_members, c.idle_renders, c.out_of_bounds, c.mismatches);
    return (c.mismatches || c.out_of_bounds || c.idle_renders) ? 1 : 0;
}
