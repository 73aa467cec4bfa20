// CPU checker of the rtx_trace_paths rules in raytrace-we-gpu_amd/csrc/rtx_paths.h
// (tests/test_paths_abi_host.py): the argument rules and their order, the
// world rules, the flag mapping, and the launch's arithmetic — the exact grid,
// which lane owns which query, and the byte offsets of a query's records —
// played out on host buffers of exactly the sizes the caller gives, so that an
// index past one is a sanitizer report. Prints one JSON line. Compiled plain
// and under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_paths.h"

namespace {

uint32_t lcg(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s;
}

// The rule written out again, independently of the header's order of tests:
// the first failing one in the order include/rtx.h lists them.
int want_args(bool q, bool r, uint32_t n, uint32_t samples, uint32_t flags, uint32_t order) {
    if (n > 0 && !q) return 1;
    if (n > 0 && !r) return 2;
    if (samples == 0) return 3;
    if (flags != 0 && flags != 1 && flags != 2 && flags != 3) return 4;
    if (order != 0 && order != 1 && order != 2) return 5;
    return 0;
}

// One launch on host memory: every lane of the exact grid, the guard, the
// query index, and the accesses k_paths makes with it. Returns the number of
// rule violations.
unsigned long long play(uint32_t n, uint32_t block, const std::vector<uint32_t> *perm, bool once,
                        unsigned long long &lanes) {
    unsigned long long bad = 0;
    std::vector<unsigned char> queries((size_t)n * rtx::kPathRayBytes, 1), results((size_t)n * rtx::kPathResultBytes, 0);
    std::vector<uint32_t> segs(n, 0u);
    const uint32_t blocks = rtx::paths_blocks(n, block);
    bad += (uint64_t)blocks * block < n || (blocks != 0 && (uint64_t)(blocks - 1) * block >= n);
    for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < block; ++t) {
            const uint64_t g64 = (uint64_t)b * block + t;
            ++lanes;
            if (!rtx::paths_lane_live(g64, n)) continue;
            const uint32_t g = (uint32_t)g64;
            const uint32_t i = rtx::paths_lane_query(g, perm != nullptr, perm ? (*perm)[g] : 0u, n);
            bad += i >= n;
            unsigned char rec[32];
            std::memcpy(rec, queries.data() + rtx::paths_query_offset(i), 32);           // two float4 loads
            results[rtx::paths_result_offset(i)] += 1;                                    // one float4 store
            std::memset(results.data() + rtx::paths_result_offset(i) + 1, rec[0], 15);
            segs[rtx::paths_segment_offset(i) / 4u] += 1u;                                // one word
        }
    if (once)  // the given order, or a permutation: every record written exactly once
        for (uint32_t i = 0; i < n; ++i) bad += results[rtx::paths_result_offset(i)] != 1 || segs[i] != 1u;
    return bad;
}

}  // namespace

int main() {
    unsigned long long arg_checks = 0, arg_bad = 0;
    const uint32_t ns[] = {0u, 1u, 64u, 0xffffffffu}, ss[] = {0u, 1u, 6u, 0xffffffffu};
    const uint32_t fs[] = {0u, 1u, 2u, 3u, 4u, 7u, 0x80000000u, 0xffffffffu}, os[] = {0u, 1u, 2u, 3u, 0xffffffffu};
    for (int q = 0; q < 2; ++q)
        for (int r = 0; r < 2; ++r)
            for (uint32_t n : ns)
                for (uint32_t s : ss)
                    for (uint32_t f : fs)
                        for (uint32_t o : os) {
                            ++arg_checks;
                            arg_bad += (int)rtx::paths_args(q != 0, r != 0, n, s, f, o) != want_args(q, r, n, s, f, o);
                        }
    arg_bad += rtx::kPathsArgOk != 0 || rtx::kPathsArgQueries != 1 || rtx::kPathsArgResults != 2 ||
               rtx::kPathsArgSamples != 3 || rtx::kPathsArgFlags != 4 || rtx::kPathsArgOrder != 5;

    // once the world is known: depth 0 first, then samples * depth < 2^32
    unsigned long long world_bad = 0;
    world_bad += rtx::paths_world(6u, 8u) != rtx::kPathsWorldOk;
    world_bad += rtx::paths_world(6u, 0u) != rtx::kPathsWorldDepth0;
    world_bad += rtx::paths_world(0xffffffffu, 0u) != rtx::kPathsWorldDepth0;
    world_bad += rtx::paths_world(65535u, 65536u) != rtx::kPathsWorldOk;
    world_bad += rtx::paths_world(65536u, 65536u) != rtx::kPathsWorldCount;
    world_bad += rtx::paths_world(0xffffffffu, 1u) != rtx::kPathsWorldOk;
    world_bad += rtx::paths_world(0xffffffffu, 2u) != rtx::kPathsWorldCount;
    world_bad += rtx::paths_world(0x80000000u, 2u) != rtx::kPathsWorldCount;
    // the guard bit alone reaches the kernel's flags; CONTINUE does not
    world_bad += rtx::paths_frame_flags(0u) != 0u || rtx::paths_frame_flags(1u) != 1u ||
                 rtx::paths_frame_flags(2u) != 0u || rtx::paths_frame_flags(3u) != 1u;

    // the exact grid at its ends (no launch this size is played out)
    unsigned long long grid_bad = 0;
    grid_bad += rtx::paths_blocks(0u, 256u) != 0u || rtx::paths_blocks(1u, 256u) != 1u ||
                rtx::paths_blocks(256u, 256u) != 1u || rtx::paths_blocks(257u, 256u) != 2u;
    grid_bad += rtx::paths_blocks(0xffffffffu, 256u) != 0x1000000u;   // n + 255 would wrap to 254
    grid_bad += rtx::paths_blocks(0xffffff01u, 256u) != 0x1000000u || rtx::paths_blocks(0xffffff00u, 256u) != 0xffffffu;
    // the last block's lanes lie past 2^32 - 1: only the 64-bit index says so
    grid_bad += rtx::paths_lane_live(0xfffffffeull, 0xffffffffu) != true;
    grid_bad += rtx::paths_lane_live(0xffffffffull, 0xffffffffu) != false;
    grid_bad += rtx::paths_lane_live(0x100000000ull, 0xffffffffu) != false;  // as 32 bits it would be lane 0
    // offsets do not wrap at i * 32 = 2^32
    grid_bad += rtx::paths_query_offset(0x08000000u) != 0x100000000ull;
    grid_bad += rtx::paths_query_offset(0xfffffffeu) != 32ull * 0xfffffffeull;
    grid_bad += rtx::paths_result_offset(0x10000000u) != 0x100000000ull;
    grid_bad += rtx::paths_segment_offset(0x40000000u) != 0x100000000ull;

    // launches played out on buffers of exactly n records
    unsigned long long lanes = 0, play_bad = 0, launches = 0;
    uint32_t s = 2024u;
    const uint32_t sizes[] = {1u, 2u, 63u, 64u, 65u, 255u, 256u, 257u, 511u, 512u, 513u, 1536u, 4099u};
    for (uint32_t n : sizes) {
        play_bad += play(n, 256u, nullptr, true, lanes);  // the given order
        std::vector<uint32_t> perm(n);
        for (uint32_t i = 0; i < n; ++i) perm[i] = i;
        for (uint32_t i = n - 1; i > 0; --i) {  // a permutation
            const uint32_t j = lcg(s) % (i + 1u);
            const uint32_t t = perm[i];
            perm[i] = perm[j];
            perm[j] = t;
        }
        play_bad += play(n, 256u, &perm, true, lanes);
        for (uint32_t i = 0; i < n; ++i) perm[i] = lcg(s);  // any words at all: clamped
        perm[0] = 0xffffffffu;
        perm[n - 1] = n;
        play_bad += play(n, 256u, &perm, false, lanes);
        launches += 3;
    }
    std::printf("{\"arg_checks\": %llu, \"arg_bad\": %llu, \"world_bad\": %llu, \"grid_bad\": %llu, "
                "\"launches\": %llu, \"lanes\": %llu, \"play_bad\": %llu, \"query_bytes\": %u, \"result_bytes\": %u, "
                "\"flag_mask\": %u}\n",
                arg_checks, arg_bad, world_bad, grid_bad, launches, lanes, play_bad, rtx::kPathRayBytes,
                rtx::kPathResultBytes, rtx::kPathsFlagMask);
    return arg_bad == 0 && world_bad == 0 && grid_bad == 0 && play_bad == 0 ? 0 : 1;
}
