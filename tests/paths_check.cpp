// CPU checker of raytrace-we-gpu_amd/csrc/rtx_paths.h (tests/test_paths_host.py):
// the seed rule against a restatement written from the reference's baseHash,
// and the sample-count rule at its boundary. Prints one JSON line. Compiled
// plain and under ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../raytrace-we-gpu_amd/csrc/rtx_paths.h"

namespace {

// baseHash(uint2 p) as ShaderCompute.hlsl:23-28 writes it, on a two-vector
void ref_hash(const uint32_t p[2], uint32_t *out) {
    uint32_t q[2];
    q[0] = 1103515245u * ((p[0] >> 1u) ^ p[1]);
    q[1] = 1103515245u * ((p[1] >> 1u) ^ p[0]);
    const uint32_t h32 = 1103515245u * (q[0] ^ (q[1] >> 3u));
    *out = h32 ^ (h32 >> 16u);
}

uint32_t lcg(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s;
}

}  // namespace

int main() {
    uint32_t s = 12345u;
    unsigned long long seed_checks = 0, seed_bad = 0, range_bad = 0;
    const uint32_t frames[] = {0u, 1u, 5u, 0x7fffffffu};
    for (int i = 0; i < 50000; ++i) {
        // small pixel coordinates, then any bit pattern
        const uint32_t x = i < 25000 ? lcg(s) % 8192u : lcg(s), y = i < 25000 ? lcg(s) % 8192u : lcg(s);
        for (const uint32_t f : frames) {
            uint32_t p[2] = {x, y}, h;
            ref_hash(p, &h);
            if (f != 0u) {
                uint32_t p2[2] = {h, 0x80000000u | f};
                ref_hash(p2, &h);
            }
            const float want = std::ldexp((float)h, -32);  // exact: a power-of-two divide
            const float got = rtx::path_seed(x, y, f);
            ++seed_checks;
            seed_bad += rtx::path_seed_hash(x, y, f) != h || !(got == want);
            range_bad += !(got >= 0.0f && got <= 1.0f);
        }
    }
    // samples * depth < 2^32
    unsigned long long count_bad = 0;
    count_bad += !rtx::paths_count_ok(1u, 1u);
    count_bad += !rtx::paths_count_ok(65535u, 65536u);
    count_bad += !rtx::paths_count_ok(0xffffffffu, 1u);
    count_bad += !rtx::paths_count_ok(1u, 0xffffffffu);
    count_bad += rtx::paths_count_ok(65536u, 65536u);
    count_bad += rtx::paths_count_ok(0xffffffffu, 2u);
    count_bad += rtx::paths_count_ok(2u, 0x80000000u);
    count_bad += rtx::paths_count_ok(0xffffffffu, 0xffffffffu);
    std::printf("{\"seed_checks\": %llu, \"seed_bad\": %llu, \"range_bad\": %llu, \"count_bad\": %llu, "
                "\"ray_bytes\": %u, \"seed_float\": %u, \"d_float\": %u}\n",
                seed_checks, seed_bad, range_bad, count_bad, rtx::kPathRayBytes, rtx::kPathRaySeed, rtx::kPathRayD);
    return seed_bad == 0 && range_bad == 0 && count_bad == 0 ? 0 : 1;
}
