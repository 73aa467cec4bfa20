// CPU checker of the rtx_trace_film rules in raytrace-we-gpu_amd/csrc/rtx_film.h
// (tests/test_film_host.py): the argument rules and their order, the record
// offsets at the ends of 32 bits, launches played out on host buffers of
// exactly the sizes the caller gives — both record sizes, with and without a
// perm — so that an index past one is a sanitizer report, and
// rtx_film_from_frame against the frame's bytes, with its refusals. Prints one
// JSON line. Compiled plain and under ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../include/rtx.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_film.h"

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
    if (flags > 7u) return 4;
    if (order != 0 && order != 1 && order != 3) return 5;
    return 0;
}

// One launch on host memory: every lane of the exact grid, the guard, the
// query index, and the accesses k_film makes with it: the record's four (six)
// float4 at a sample start, one float4 result, one segment word.
unsigned long long play(uint32_t n, uint32_t block, bool lens, const std::vector<uint32_t> *perm, bool once,
                        unsigned long long &lanes) {
    unsigned long long bad = 0;
    const uint32_t rec_bytes = rtx::film_record_bytes(lens);
    std::vector<unsigned char> queries((size_t)n * rec_bytes, 1), results((size_t)n * rtx::kPathResultBytes, 0);
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
            bad += rtx::film_query_vec4(i, lens) * 16u != rtx::film_query_offset(i, lens);
            unsigned char rec[96];
            for (uint32_t k = 0; k < rtx::film_record_vec4(lens); ++k)  // the float4 loads of a sample start
                std::memcpy(rec + 16 * k, queries.data() + (rtx::film_query_vec4(i, lens) + k) * 16u, 16);
            results[rtx::film_result_offset(i)] += 1;  // one float4 store
            std::memset(results.data() + rtx::film_result_offset(i) + 1, rec[rec_bytes - 1], 15);
            segs[rtx::film_segment_offset(i) / 4u] += 1u;  // one word
        }
    if (once)  // the given order, or a permutation: every record written exactly once
        for (uint32_t i = 0; i < n; ++i) bad += results[rtx::film_result_offset(i)] != 1 || segs[i] != 1u;
    return bad;
}

}  // namespace

int main() {
    unsigned long long arg_checks = 0, arg_bad = 0, offset_bad = 0, launches = 0, play_bad = 0, lanes = 0, frame_bad = 0,
                       frame_records = 0, refusal_bad = 0;
    // the argument rules, first failure first
    const uint32_t ns[] = {0u, 1u, 5u, 0xFFFFFFFFu}, samples[] = {0u, 1u, 6u, 0xFFFFFFFFu};
    const uint32_t flags[] = {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 15u, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t orders[] = {0u, 1u, 2u, 3u, 4u, 0xFFFFFFFFu};
    for (int q = 0; q < 2; ++q)
        for (int r = 0; r < 2; ++r)
            for (uint32_t n : ns)
                for (uint32_t s : samples)
                    for (uint32_t f : flags)
                        for (uint32_t o : orders) {
                            ++arg_checks;
                            arg_bad += (int)rtx::film_args(q != 0, r != 0, n, s, f, o) != want_args(q != 0, r != 0, n, s, f, o);
                        }
    // the offsets near 2^32: no wrap in either record size
    for (uint32_t i : {0u, 1u, (1u << 26) - 1u, 1u << 26, 44739243u, 1u << 27, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
        offset_bad += rtx::film_query_offset(i, false) != (uint64_t)i * 64u || rtx::film_query_offset(i, true) != (uint64_t)i * 96u;
        offset_bad += rtx::film_query_vec4(i, false) != (uint64_t)i * 4u || rtx::film_query_vec4(i, true) != (uint64_t)i * 6u;
        offset_bad += rtx::film_result_offset(i) != (uint64_t)i * 16u || rtx::film_segment_offset(i) != (uint64_t)i * 4u;
    }
    offset_bad += rtx::paths_blocks(0xFFFFFFFFu, 256u) != (1u << 24) || rtx::paths_lane_live(1ull << 32, 0xFFFFFFFFu);
    offset_bad += !rtx::paths_lane_live(0xFFFFFFFEull, 0xFFFFFFFFu);
    // launches on buffers of exactly n records
    uint32_t seed = 12345u;
    for (int lens = 0; lens < 2; ++lens)
        for (uint32_t n : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 4099u}) {
            play_bad += play(n, 256u, lens != 0, nullptr, true, lanes);
            std::vector<uint32_t> perm(n);
            for (uint32_t i = 0; i < n; ++i) perm[i] = i;
            for (uint32_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[lcg(seed) % (i + 1)]);
            play_bad += play(n, 256u, lens != 0, &perm, true, lanes);
            for (uint32_t i = 0; i < n; ++i) perm[i] = lcg(seed);  // arbitrary words: clamped, never outside
            play_bad += play(n, 256u, lens != 0, &perm, false, lanes);
            launches += 3;
        }
    // rtx_film_from_frame against the frame's bytes
    rtx_frame f;
    std::memset(&f, 0, sizeof(f));
    float *rows[6] = {f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v};
    for (int k = 0; k < 6; ++k)
        for (int j = 0; j < 4; ++j) rows[k][j] = (float)(10 * k + j) + 0.25f;
    f.lens_u[3] = 0.0f;
    f.width = 7;
    f.height = 5;
    f.img_w = 7.5f;
    f.img_h = 4.25f;
    for (int lens = 0; lens < 2; ++lens) {
        f.lens_u[3] = lens ? 0.125f : 0.0f;
        std::vector<uint32_t> xs, ys;
        for (uint32_t y = 0; y < f.height; ++y)
            for (uint32_t x = 0; x < f.width; ++x) {
                xs.push_back(f.width - 1 - x);
                ys.push_back(y);
            }
        const uint32_t n = (uint32_t)xs.size();
        std::vector<unsigned char> out((size_t)n * (lens ? 96 : 64), 0xA5);  // exactly n records
        const auto rc = rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, f.width,
                                             f.height, f.rng_mode, xs.data(), ys.data(), n, 3u, out.data(), lens != 0);
        frame_bad += rc != rtx::kFilmFrameOk;
        for (uint32_t i = 0; i < n; ++i) {
            float r[24] = {};
            uint32_t w[24];
            std::memcpy(r, out.data() + (size_t)i * (lens ? 96 : 64), lens ? 96 : 64);
            std::memcpy(w, r, sizeof(w));
            ++frame_records;
            frame_bad += std::memcmp(r + 0, f.origin, 12) != 0 || std::memcmp(r + 4, f.lower_left, 12) != 0;
            frame_bad += std::memcmp(r + 8, f.horizontal, 12) != 0 || std::memcmp(r + 12, f.vertical, 12) != 0;
            const float s = rtx::path_seed(xs[i], ys[i], 3u);
            frame_bad += std::memcmp(r + 3, &s, 4) != 0 || w[7] != 0u;
            frame_bad += r[11] != (float)xs[i] || r[15] != (float)ys[i];
            if (lens) frame_bad += std::memcmp(r + 16, f.lens_u, 16) != 0 || std::memcmp(r + 20, f.lens_v, 12) != 0 || w[23] != 0u;
        }
    }
    {  // the refusals, in order; nothing is written by a refused call
        unsigned char out[96 * 2];
        std::memset(out, 0xA5, sizeof(out));
        const uint32_t x0[2] = {0, 6}, y0[2] = {0, 4}, xb[2] = {0, 7}, yb[2] = {5, 0};
        f.lens_u[3] = 0.125f;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0, x0,
                                            y0, 2, 0, out, false) != rtx::kFilmFrameLens;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 1, x0,
                                            y0, 2, 0, out, false) != rtx::kFilmFrameRng;  // the RNG rule comes first
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 1, x0,
                                            y0, 2, 0, out, true) != rtx::kFilmFrameRng;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0, xb,
                                            y0, 2, 0, out, true) != rtx::kFilmFramePixel;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0, x0,
                                            yb, 2, 0, out, true) != rtx::kFilmFramePixel;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0,
                                            nullptr, y0, 2, 0, out, true) != rtx::kFilmFrameNull;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0, x0,
                                            y0, 2, 0, nullptr, true) != rtx::kFilmFrameNull;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0,
                                            nullptr, nullptr, 0, 0, nullptr, true) != rtx::kFilmFrameOk;  // an empty list
        for (unsigned char c : out) refusal_bad += c != 0xA5;
        refusal_bad += rtx::film_from_frame(f.origin, f.horizontal, f.vertical, f.lower_left, f.lens_u, f.lens_v, 7, 5, 0, x0,
                                            y0, 2, 0, out, true) != rtx::kFilmFrameOk;
    }
    std::printf("{\"arg_checks\": %llu, \"arg_bad\": %llu, \"offset_bad\": %llu, \"launches\": %llu, \"play_bad\": %llu, "
                "\"lanes\": %llu, \"frame_records\": %llu, \"frame_bad\": %llu, \"refusal_bad\": %llu, "
                "\"query_bytes\": %u, \"lens_query_bytes\": %u, \"flag_mask\": %u, \"struct_bytes\": [%zu, %zu]}\n",
                arg_checks, arg_bad, offset_bad, launches, play_bad, lanes, frame_records, frame_bad, refusal_bad,
                rtx::kFilmBytes, rtx::kFilmLensBytes, rtx::kFilmFlagMask, sizeof(rtx_film_query), sizeof(rtx_film_lens_query));
    return (arg_bad | offset_bad | play_bad | frame_bad | refusal_bad) != 0 ? 1 : 0;
}
