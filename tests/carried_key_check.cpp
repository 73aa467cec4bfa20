// carried_key_check.cpp — CPU checker of the carried queue key and the host's
// fallback rule (raytrace-we-gpu_amd/csrc/rtx_refine_keys.h), the text the
// kernels and rtx_refine run. Stand-alone: its own main, no HIP, no library.
// Prints one JSON line; exit status 0 iff every check held.
//
//   1. carried_key == the pre-pass's cost_key formula (restated below from
//      rtx_kernels.hip, sat_cap = 0) for s_prev = kCostSpp and 1 on random maps,
//      1-pixel-wide and 1-row images included (edge clamping)
//   2. the key never increases when any window entry grows
//   3. the top bucket (key 0), no overflow, at the largest counts the host
//      rule admits: entries of 2^32 - 1 with s_prev = 1 and s_prev = 2^32 - 1
//   4. the host's fallback rule on a table of cases
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_refine_keys.h"

using namespace rtx;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

// cost_key of rtx_kernels.hip with sat_cap = 0, 32-bit as there (the maps of
// check 1 keep its sums far below 2^32)
static uint32_t cost_key_ref(const uint32_t *cost, uint32_t i, uint32_t width, uint32_t rows, uint32_t cost_spp) {
    const int x = (int)(i % width), y = (int)(i / width);
    uint32_t sum = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy < 0 ? 0 : (y + dy > (int)rows - 1 ? (int)rows - 1 : y + dy);
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx < 0 ? 0 : (x + dx > (int)width - 1 ? (int)width - 1 : x + dx);
            sum += cost[(uint32_t)yy * width + (uint32_t)xx];
        }
    }
    const uint32_t win = 9u * cost_spp;
    if (win != 9u) sum = (sum * 9u + win / 2u) / win;
    return (kCostBuckets - 1u) - (sum < kCostBuckets - 1u ? sum : kCostBuckets - 1u);
}

int main() {
    unsigned long long equal_checks = 0, equal_bad = 0, mono_checks = 0, mono_bad = 0;
    unsigned top_checks = 0, top_bad = 0, rule_cases = 0, rule_bad = 0;

    // 1. equality with the pre-pass formula
    const uint32_t shapes[][2] = {{7, 5}, {1, 9}, {9, 1}, {1, 1}, {2, 2}, {16, 3}, {33, 17}};
    const uint32_t spps[] = {kCostSpp, 1u};
    for (const auto &sh : shapes) {
        const uint32_t w = sh[0], h = sh[1];
        for (uint32_t s_prev : spps) {
            for (int rep = 0; rep < 8; ++rep) {
                // segment counts of s_prev samples: from all-cheap to around the
                // top bucket (a window sum of 255 * s_prev) and beyond
                const uint32_t hi = (rep < 3 ? 8u : rep < 6 ? 60u : 400u) * s_prev;
                std::vector<uint32_t> m((size_t)w * h);
                for (auto &v : m) v = rnd() % (hi + 1u);
                for (uint32_t i = 0; i < w * h; ++i) {
                    ++equal_checks;
                    if (carried_key(m.data(), i, w, h, s_prev) != cost_key_ref(m.data(), i, w, h, s_prev)) ++equal_bad;
                }
            }
        }
    }

    // 2. monotone: growing any entry of the window never raises the key
    for (int rep = 0; rep < 400; ++rep) {
        const uint32_t w = 1u + rnd() % 6u, h = 1u + rnd() % 6u;
        const uint32_t s_prev = rep % 3 == 0 ? 1u : rep % 3 == 1 ? 1u + rnd() % 100u : 0xffffffffu - rnd() % 1000u;
        std::vector<uint32_t> m((size_t)w * h);
        for (auto &v : m) v = rep % 2 ? rnd() : rnd() % (300u * (s_prev < 1000u ? s_prev : 1000u));
        const uint32_t i = rnd() % (w * h);
        const uint32_t before = carried_key(m.data(), i, w, h, s_prev);
        for (uint32_t j = 0; j < w * h; ++j) {
            std::vector<uint32_t> g = m;
            const uint32_t room = 0xffffffffu - g[j];
            g[j] += room ? 1u + rnd() % room : 0u;
            ++mono_checks;
            if (carried_key(g.data(), i, w, h, s_prev) > before) ++mono_bad;
        }
    }

    // 3. the largest counts the host rule admits (samples * depth < 2^32, so
    // an entry is at most 2^32 - 1)
    {
        const uint32_t big[] = {0xffffffffu, 0xfffffffeu, 0xffffff00u};
        for (uint32_t e : big) {
            for (const auto &sh : shapes) {
                std::vector<uint32_t> m((size_t)sh[0] * sh[1], e);
                for (uint32_t i = 0; i < sh[0] * sh[1]; ++i) {
                    // one sample each: far above the top bucket's 255
                    ++top_checks;
                    if (carried_key(m.data(), i, sh[0], sh[1], 1u) != 0u) ++top_bad;
                    // 2^32 - 1 samples: about one segment per sample, the 9-window
                    // sums to 9 (to within rounding): bucket 255 - 9, not wrapped
                    ++top_checks;
                    const uint32_t k = carried_key(m.data(), i, sh[0], sh[1], 0xffffffffu);
                    if (k != kCostBuckets - 1u - 9u) ++top_bad;
                }
            }
        }
        // and with 300 segments per sample over 2^32 - 1 samples' worth of
        // entries the count cannot be represented: the rule refuses such a map
        ++top_checks;
        if (cost_map_fits(0xffffffffu, 300u)) ++top_bad;
    }

    // 4. the host's rule: {mode, s_prev, samples, large scene} -> carried?
    struct Case {
        int mode;
        uint32_t s_prev, samples;
        bool large, want;
    };
    const Case cases[] = {
        {kKeysCarried, 9, 12, false, true},                  // the ordinary carried step
        {kKeysPrepass, 9, 12, false, false},                 // the default mode never carries
        {kKeysCarried, 0, 12, false, false},                 // no valid map
        {kKeysCarried, 9, kLptMinSpp - 1, false, false},     // an unscheduled step
        {kKeysCarried, 9, kLptMinSpp, false, true},          // the smallest scheduled step
        {kKeysCarried, kCostSpp - 1, 12, false, false},      // covers less than a small-scene pre-pass
        {kKeysCarried, kCostSpp, 12, false, true},           // ... exactly as much
        {kKeysCarried, 3, 9, false, true},                   // an exact-grid step's map is enough
        {kKeysCarried, kCostSppLarge, 10, true, true},       // large scenes: one sample is enough
        {kKeysCarried, kCostSppLarge, 10, false, kCostSppLarge >= kCostSpp},
        {kKeysCarried, 0xffffffffu, 0xffffffffu, true, true},
        {kKeysUnscheduled, 9, 12, false, false},             // not a mode
        {7, 9, 12, false, false},
    };
    for (const Case &c : cases) {
        ++rule_cases;
        if (launch_is_carried(c.mode, c.s_prev, c.samples, c.large) != c.want) ++rule_bad;
    }
    // map validity after a launch of (samples, depth)
    struct After {
        uint32_t samples, depth, want;
    };
    const After after[] = {
        {12, 50, 12},          {1, 1, 1},           {12, 0, 0},                   // depth 0 traces nothing
        {0x10000u, 0x10000u, 0},                                                  // samples * depth == 2^32
        {0xffffu, 0x10001u, 0xffffu},                                             // 2^32 - 1
        {0xffffffffu, 1, 0xffffffffu}, {0xffffffffu, 2, 0}, {0x80000000u, 2, 0},
    };
    for (const After &a : after) {
        ++rule_cases;
        if (cost_map_after(a.samples, a.depth) != a.want) ++rule_bad;
    }

    std::printf("{\"equal_checks\": %llu, \"equal_bad\": %llu, \"mono_checks\": %llu, \"mono_bad\": %llu, "
                "\"top_checks\": %u, \"top_bad\": %u, \"rule_cases\": %u, \"rule_bad\": %u}\n",
                equal_checks, equal_bad, mono_checks, mono_bad, top_checks, top_bad, rule_cases, rule_bad);
    return equal_bad || mono_bad || top_bad || rule_bad ? 1 : 0;
}
