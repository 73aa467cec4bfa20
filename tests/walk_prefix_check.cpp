// walk_prefix_check.cpp — CPU check of the item prefix of the wave-cooperative
// walk (raytrace-we-gpu_amd/csrc/rtx_grid.h grid_item_prefix, as
// rtx_kernels.hip grid_wave_mask calls it), with the header's own code.
//
// For a wave of 64 lanes with item counts n[l] <= kGridMaxSteps and a set of
// active lanes, every active lane's start must be the plain exclusive prefix
// sum of n over the active lanes before it and total the plain sum: with 1,
// 17 and 64 active lanes, every n 0, one lane with 48 and the rest 0, every
// lane with 48, counts that stay below 8 (the high bits are then skipped),
// counts of exactly 7 and 8, and random waves. The ballots are emulated as
// masks over the active lanes; an inactive lane's n is garbage and must not
// count.
// Prints one JSON line; exit status 1 on any difference.
// Build: g++ -O2 -std=c++17 walk_prefix_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"

static unsigned long long g_s = 0x2545f4914f6cdd1dull;
static uint32_t rnd() {
    g_s ^= g_s << 13, g_s ^= g_s >> 7, g_s ^= g_s << 17;
    return (uint32_t)(g_s >> 32);
}

static long g_waves = 0, g_wrong = 0, g_skipped_high = 0;

static void check(const uint32_t *n, uint64_t act) {
    ++g_waves;
    bool any_high = false;
    for (int l = 0; l < 64; ++l) any_high |= ((act >> l) & 1u) && n[l] >= 8u;
    g_skipped_high += !any_high;
    auto bits = [&](uint32_t b) {
        uint64_t m = 0;
        for (int l = 0; l < 64; ++l)
            if (((act >> l) & 1u) && ((n[l] >> b) & 1u)) m |= 1ull << l;
        return m;
    };
    uint32_t sum = 0;
    bool bad = false;
    uint32_t total_seen = 0;
    for (int l = 0; l < 64; ++l) {
        if (!((act >> l) & 1u)) continue;
        uint32_t start, total;
        rtx::grid_item_prefix(bits, any_high,
                              [&](uint64_t m) { return (uint32_t)__builtin_popcountll(m & ((1ull << l) - 1ull)); },
                              start, total);
        bad |= start != sum;
        sum += n[l];
        total_seen = total;
    }
    if (act != 0ull) bad |= total_seen != sum;
    g_wrong += bad;
}

int main() {
    uint32_t n[64];
    const uint32_t kMax = rtx::kGridMaxSteps;
    const uint64_t acts[] = {1ull << 37, 1ull, 1ull << 63, 0x1ffffull, 0xaaaaaaaa55555555ull & 0x0003ffff0001ffffull,
                             ~0ull, 0x00000000ffffffffull, 0xffff0000ffff0000ull};
    for (uint64_t act : acts) {
        for (int shape = 0; shape < 8; ++shape) {
            for (int l = 0; l < 64; ++l) {
                const bool on = (act >> l) & 1u;
                uint32_t v = 0;
                switch (shape) {
                    case 0: v = 0; break;
                    case 1: v = kMax; break;
                    case 2: v = l == (int)(__builtin_ctzll(act) + (__builtin_popcountll(act) > 20 ? 19 : 0)) ? kMax : 0; break;
                    case 3: v = rnd() % 8u; break;
                    case 4: v = 7; break;
                    case 5: v = (l % 5 == 0) ? 8 : 7; break;
                    case 6: v = rnd() % (kMax + 1u); break;
                    default: v = (rnd() % 16u == 0) ? rnd() % (kMax + 1u) : rnd() % 3u; break;
                }
                n[l] = on ? v : rnd();  // an inactive lane's register holds anything
            }
            check(n, act);
        }
    }
    for (int w = 0; w < 200000; ++w) {
        const uint64_t act = (((uint64_t)rnd() << 32) | rnd()) | (w % 3 == 0 ? ~0ull : 0ull);
        const uint32_t cap = (w % 2) ? 7u : kMax;
        for (int l = 0; l < 64; ++l) n[l] = ((act >> l) & 1u) ? rnd() % (cap + 1u) : rnd();
        check(n, act);
    }
    std::printf("{\"waves\": %ld, \"waves_wrong\": %ld, \"waves_without_high_bits\": %ld, \"max_items\": %u}\n", g_waves,
                g_wrong, g_skipped_high, kMax);
    return g_wrong != 0 || kMax >= 64u;
}
