// adaptive_check.cpp — CPU checker of the adaptive refinement rule
// (raytrace-we-gpu_amd/csrc/rtx_adaptive.h), the text the kernels and
// rtx_refine_adaptive run. Stand-alone: its own main, no HIP, no library.
// Build with -ffp-contract=off. Prints one JSON line; exit status 0 iff every
// check held.
//
//   1. E is +inf at n_old == 0, whatever the sums
//   2. NaN sums give a NaN E
//   3. E equals an op-by-op restatement (every intermediate forced through a
//      volatile float) on random and extreme inputs, bit for bit
//   4. the mask equals a brute-force restatement on images 1x1, 1x5, 5x1, 3x3
//      and 17x9 with random errors (NaN and +inf entries included), thresholds
//      (+inf included) and caps
//   5. the argument rules
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_adaptive.h"

using namespace rtx;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static float unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

static float err_of(const float *so, uint32_t n0, const float *sn, uint32_t n1) {
    return adaptive_error_with(so, n0, sn, n1, [](float v) { return sqrtf(v); });
}

// the restatement: one IEEE operation per statement, each result stored
static float err_ref(const float *so, uint32_t n0, const float *sn, uint32_t n1) {
    if (n0 == 0u) return std::numeric_limits<float>::infinity();
    volatile float a = (float)n0, b = (float)n1, sf = (float)(n1 - n0);
    volatile float m0[3], m1[3], ad[3];
    for (int c = 0; c < 3; ++c) {
        m0[c] = so[c] / a;
        m1[c] = sn[c] / b;
        volatile float df = m1[c] - m0[c];
        ad[c] = std::fabs(df);
    }
    volatile float d01 = ad[0] + ad[1];
    volatile float d = d01 + ad[2];
    volatile float l01 = m1[0] + m1[1];
    volatile float l = l01 + m1[2];
    volatile float ratio = a / sf;
    volatile float r = std::sqrt(ratio);
    volatile float num = d * r;
    volatile float lp = l + 0.01f;
    volatile float den = std::sqrt(lp);
    volatile float e = num / den;
    return e;
}

static bool active_ref(const std::vector<float> &err, const std::vector<uint32_t> &count, int x, int y, int w, int h,
                       uint32_t samples, float thr, uint32_t cap) {
    bool noisy = false;
    for (int yy = 0; yy < h; ++yy)
        for (int xx = 0; xx < w; ++xx)
            if (std::abs(xx - x) <= 1 && std::abs(yy - y) <= 1 && err[(size_t)yy * w + xx] >= thr) noisy = true;
    const bool room = cap == 0u || (uint64_t)count[(size_t)y * w + x] + samples <= cap;
    return noisy && room;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    unsigned inf_checks = 0, inf_bad = 0, nan_checks = 0, nan_bad = 0, arg_cases = 0, arg_bad = 0;
    unsigned long long eq_checks = 0, eq_bad = 0, mask_checks = 0, mask_bad = 0, mask_on = 0;

    // 1. n_old == 0
    for (int k = 0; k < 64; ++k) {
        const float so[3] = {k & 1 ? nan : unit(), unit(), k & 2 ? inf : unit()};
        const float sn[3] = {unit() * 100.0f, k & 4 ? nan : unit(), unit()};
        const float e = err_of(so, 0u, sn, 1u + rnd() % 1000u);
        ++inf_checks;
        if (!(e == inf)) ++inf_bad;
    }
    // 2. NaN in any sum
    for (int k = 0; k < 6; ++k) {
        float so[3] = {1.0f, 2.0f, 3.0f}, sn[3] = {2.0f, 4.0f, 6.5f};
        (k < 3 ? so : sn)[k % 3] = nan;
        ++nan_checks;
        if (!std::isnan(err_of(so, 8u, sn, 16u))) ++nan_bad;
    }
    // 3. against the restatement
    const float extreme[] = {0.0f, 1e-45f, 1.17549435e-38f, 1e-20f, 0.01f, 1.0f, 3.0f, 1e10f, 3.4e38f, inf, -0.01f, -1.0f};
    const uint32_t counts[] = {1u, 2u, 3u, 8u, 16u, 17u, 1000u, 16777217u, 0x7fffffffu, 0xfffffffeu};
    for (float s0 : extreme)
        for (float s1 : extreme)
            for (uint32_t n0 : counts)
                for (uint32_t step : {1u, 8u, 0x80000000u}) {
                    if (step > 0xffffffffu - n0) continue;
                    const float so[3] = {s0, s1, s0}, sn[3] = {s1, s0 + s1, s1};
                    ++eq_checks;
                    if (!same(err_of(so, n0, sn, n0 + step), err_ref(so, n0, sn, n0 + step))) ++eq_bad;
                }
    for (int k = 0; k < 200000; ++k) {
        const uint32_t n0 = 1u + rnd() % 4096u, step = 1u + rnd() % 64u;
        float so[3], sn[3];
        for (int c = 0; c < 3; ++c) {
            so[c] = unit() * (float)n0;
            sn[c] = so[c] + unit() * (float)step * (k & 1 ? 1.0f : 20.0f);
        }
        ++eq_checks;
        if (!same(err_of(so, n0, sn, n0 + step), err_ref(so, n0, sn, n0 + step))) ++eq_bad;
    }
    // 4. the mask
    const int shapes[][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 3}, {17, 9}};
    for (const auto &sh : shapes) {
        const int w = sh[0], h = sh[1];
        for (int rep = 0; rep < 40; ++rep) {
            std::vector<float> err((size_t)w * h);
            std::vector<uint32_t> count((size_t)w * h);
            for (size_t i = 0; i < err.size(); ++i) {
                const uint32_t r = rnd() % 16u;
                err[i] = r == 0u ? nan : r == 1u ? inf : r < 10u ? unit() * 0.1f : unit();
                count[i] = 8u * (1u + rnd() % 6u);
            }
            const float thr = rep % 8 == 0 ? inf : rep % 8 == 1 ? 0.0f : unit();
            const uint32_t samples = rep % 3 == 0 ? 3u : 8u;
            const uint32_t cap = rep % 4 == 0 ? 0u : rep % 4 == 1 ? 0xffffffffu : 8u * (2u + rnd() % 6u);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const bool got = adaptive_active(err.data(), count.data(), (uint32_t)(y * w + x), (uint32_t)w,
                                                     (uint32_t)h, samples, thr, cap);
                    ++mask_checks;
                    mask_on += got;
                    if (got != active_ref(err, count, x, y, w, h, samples, thr, cap)) ++mask_bad;
                }
        }
    }
    {  // a count near 2^32: the cap's sum does not wrap
        const float e1[1] = {inf};
        const uint32_t c1[1] = {0xfffffff0u};
        ++mask_checks;
        if (adaptive_active(e1, c1, 0u, 1u, 1u, 32u, 0.5f, 0xffffffffu)) ++mask_bad;
        ++mask_checks;
        if (!adaptive_active(e1, c1, 0u, 1u, 1u, 15u, 0.5f, 0xffffffffu)) ++mask_bad;
    }
    // 5. the argument rules
    const struct {
        uint32_t s;
        float t;
        uint32_t m;
        bool ok;
    } args[] = {{8u, 0.1f, 0u, true},  {8u, inf, 0u, true},   {8u, -1.0f, 8u, true}, {1u, 0.0f, 0xffffffffu, true},
                {0u, 0.1f, 0u, false}, {8u, nan, 0u, false},  {8u, 0.1f, 7u, false}, {0u, nan, 1u, false}};
    for (const auto &a : args) {
        ++arg_cases;
        if ((adaptive_args_error(a.s, a.t, a.m) == nullptr) != a.ok) ++arg_bad;
    }
    std::printf("{\"inf_checks\": %u, \"inf_bad\": %u, \"nan_checks\": %u, \"nan_bad\": %u, \"eq_checks\": %llu, "
                "\"eq_bad\": %llu, \"mask_checks\": %llu, \"mask_bad\": %llu, \"mask_on\": %llu, \"arg_cases\": %u, "
                "\"arg_bad\": %u}\n",
                inf_checks, inf_bad, nan_checks, nan_bad, eq_checks, eq_bad, mask_checks, mask_bad, mask_on, arg_cases,
                arg_bad);
    return inf_bad || nan_bad || eq_bad || mask_bad || arg_bad ? 1 : 0;
}
