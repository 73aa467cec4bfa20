// features_check.cpp — CPU checker of the feature buffers' rules
// (raytrace-we-gpu_amd/csrc/rtx_features.h), the text the kernels, rtx_pick and
// rtx_mask_from_ids run. Stand-alone: its own main, no HIP, no library. Build
// with -ffp-contract=off. Prints one JSON line; exit status 0 iff every check
// held.
//
//   1. the pixel-centre ray equals an op-by-op restatement (every intermediate
//      forced through a volatile float) on random frames and pixels
//   2. depth equals its restatement, and is +inf for t = +inf
//   3. the id mask (feature_id_listed, then feature_mask_grown) equals a brute
//      force over all pixel pairs on images 1x1, 1x5, 5x1 and 17x9, grow 0, 1,
//      3 and 8, lists of 1 and 256 ids, with ids nobody shows and the entry
//      0xffffffff ("-1") in the list, misses (-1) in the plane
//   4. the masked rule's cap, near 2^32 included
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_features.h"

using namespace rtx;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static float unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static float span(float lo, float hi) { return lo + (hi - lo) * unit(); }
static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

// the restatements: one IEEE operation per statement, each result stored
static void ray_ref(const float *org, const float *hor, const float *ver, const float *llc, float img_w, float img_h,
                    uint32_t x, uint32_t y, float *d) {
    volatile float xf = (float)x, yf = (float)y;
    volatile float xc = xf + 0.5f, yc = yf + 0.5f;
    volatile float wm = img_w - 1.0f, hm = img_h - 1.0f;
    volatile float u = xc / wm, v = yc / hm;
    for (int k = 0; k < 3; ++k) {
        volatile float uh = u * hor[k];
        volatile float a = llc[k] + uh;
        volatile float vv = v * ver[k];
        volatile float b = a + vv;
        volatile float c = b - org[k];
        d[k] = c;
    }
}
static float depth_ref(float t, const float *d) {
    volatile float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
    volatile float xy = xx + yy;
    volatile float s = xy + zz;
    volatile float l = sqrtf(s);
    volatile float r = t * l;
    return r;
}

int main() {
    long ray_checks = 0, ray_bad = 0, depth_checks = 0, depth_bad = 0;
    for (int it = 0; it < 100000; ++it) {
        float org[3], hor[3], ver[3], llc[3];
        for (int k = 0; k < 3; ++k) {
            org[k] = span(-20.0f, 20.0f);
            hor[k] = span(-8.0f, 8.0f);
            ver[k] = span(-8.0f, 8.0f);
            llc[k] = span(-20.0f, 20.0f);
        }
        const uint32_t w = 2u + rnd() % 4000u, h = 2u + rnd() % 3000u;
        const float img_w = (float)w, img_h = (it & 1) ? (float)w / span(0.5f, 3.0f) : (float)h;
        const uint32_t x = rnd() % w, y = rnd() % h;
        float d[3], r[3];
        feature_ray(org, hor, ver, llc, img_w, img_h, x, y, d);
        ray_ref(org, hor, ver, llc, img_w, img_h, x, y, r);
        ++ray_checks;
        if (!(same(d[0], r[0]) && same(d[1], r[1]) && same(d[2], r[2]))) ++ray_bad;
        const float t = (it % 97 == 0) ? std::numeric_limits<float>::infinity() : span(0.001f, 2000.0f);
        const float got = feature_depth(t, d, [](float v) { return sqrtf(v); });
        ++depth_checks;
        if (!same(got, depth_ref(t, d))) ++depth_bad;
        if (std::isinf(t) && !(std::isinf(got) && got > 0.0f)) ++depth_bad;
    }

    // the id mask against a brute force over all pixel pairs
    long mask_checks = 0, mask_bad = 0, mask_on = 0, listed_on = 0, miss_listed = 0;
    const uint32_t shapes[4][2] = {{1, 1}, {1, 5}, {5, 1}, {17, 9}};
    const uint32_t grows[4] = {0, 1, 3, 8};
    const uint32_t counts[2] = {1, 256};
    for (const auto &sh : shapes)
        for (uint32_t grow : grows)
            for (uint32_t n : counts)
                for (int rep = 0; rep < 10; ++rep) {
                    const uint32_t W = sh[0], H = sh[1];
                    // the plane: indices below `range`, about a fifth misses
                    const uint32_t range = n == 1 ? 6u : 1200u;
                    std::vector<float> surf(4 * (size_t)W * H, 0.5f);
                    for (uint32_t i = 0; i < W * H; ++i)
                        surf[4 * i + 3] = rnd() % 5u == 0u ? -1.0f : (float)(rnd() % range);
                    // the list: shown ids, ids beyond every index (absent), and "-1"
                    std::vector<uint32_t> ids(n);
                    for (uint32_t k = 0; k < n; ++k) ids[k] = rnd() % 4u == 0u ? range + rnd() % 1000u : rnd() % range;
                    if (n > 1) ids[rnd() % n] = 0xffffffffu;
                    if (n == 1 && rep % 3 == 1) ids[0] = 0xffffffffu;
                    if (n == 1 && rep % 3 == 2) ids[0] = range + 7u;
                    std::vector<uint8_t> listed((size_t)W * H);
                    for (uint32_t i = 0; i < W * H; ++i) {
                        listed[i] = feature_id_listed(surf[4 * i + 3], ids.data(), n) ? 1 : 0;
                        listed_on += listed[i];
                        if (listed[i] && surf[4 * i + 3] < 0.0f) ++miss_listed;
                    }
                    for (uint32_t i = 0; i < W * H; ++i) {
                        const bool got = feature_mask_grown(listed.data(), i, W, H, grow);
                        bool want = false;
                        const long xi = i % W, yi = i / W;
                        for (uint32_t q = 0; q < W * H && !want; ++q) {
                            const long xq = q % W, yq = q / W;
                            const long dx = std::labs(xq - xi), dy = std::labs(yq - yi);
                            if ((dx > dy ? dx : dy) > (long)grow) continue;
                            const float wq = surf[4 * q + 3];
                            if (wq < 0.0f) continue;  // a miss shows nothing
                            for (uint32_t k = 0; k < n && !want; ++k) want = (double)ids[k] == (double)wq;
                        }
                        ++mask_checks;
                        mask_on += got;
                        if (got != want) ++mask_bad;
                    }
                }
    // NaN, negative and huge ids in the plane are never listed
    const uint32_t any[3] = {0u, 0xffffffffu, 0x7fffffffu};
    long odd_bad = 0;
    const float odd[5] = {std::nanf(""), -1.0f, -0.5f, 4294967296.0f, std::numeric_limits<float>::infinity()};
    for (float w : odd)
        if (feature_id_listed(w, any, 3)) ++odd_bad;
    if (!feature_id_listed(0.0f, any, 3)) ++odd_bad;

    // the masked rule
    long cap_cases = 0, cap_bad = 0;
    struct Cap { uint8_t m; uint32_t count, samples, cap; bool want; };
    const Cap caps[] = {{0, 0, 8, 0, false},        {1, 0, 8, 0, true},          {255, 16, 8, 24, true},
                        {1, 17, 8, 24, false},      {1, 24, 8, 24, false},       {1, 0xfffffff0u, 0x20u, 0xffffffffu, false},
                        {1, 0xfffffff0u, 0xfu, 0xffffffffu, true}, {0, 0, 8, 24, false}};
    for (const Cap &c : caps) {
        ++cap_cases;
        if (masked_active(c.m, c.count, c.samples, c.cap) != c.want) ++cap_bad;
    }

    std::printf("{\"ray_checks\": %ld, \"ray_bad\": %ld, \"depth_checks\": %ld, \"depth_bad\": %ld, "
                "\"mask_checks\": %ld, \"mask_bad\": %ld, \"mask_on\": %ld, \"listed_on\": %ld, \"miss_listed\": %ld, "
                "\"odd_bad\": %ld, \"cap_cases\": %ld, \"cap_bad\": %ld}\n",
                ray_checks, ray_bad, depth_checks, depth_bad, mask_checks, mask_bad, mask_on, listed_on, miss_listed,
                odd_bad, cap_cases, cap_bad);
    return (ray_bad || depth_bad || mask_bad || miss_listed || odd_bad || cap_bad) ? 1 : 0;
}
