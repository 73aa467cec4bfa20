// layout_blocks.h — how many flat blocks the layer grid marks per ray and per
// wave of 64 rays, for a given order of the layer's spheres (rtx_layout.h).
// Shared by tools/layout_blocks.cpp (the tool that chooses the order) and
// tests/layout_check.cpp. The grids are built and walked by the project's own
// headers; a ray's mask is grid_mask_items, what the kernel's wave computes
// (rtx_kernels.hip grid_wave_mask), and a wave's is the OR over its live lanes.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_layout.h"

namespace lb {

struct Ray {
    float o[3], d[3];
    bool live;
};

struct Rng {
    unsigned long long s;
    explicit Rng(unsigned long long seed) : s(seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull) {}
    double uni() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
    double sym() { return 2.0 * uni() - 1.0; }
};

// The seeded synthetic family: waves of 64 lanes, each wave a 16 x 4 pixel
// patch of a 1920 x 1080 frame of the RTIOW camera (from (13, 2, 3) towards
// the origin, vfov 20). A lane is at a random segment of its path: the primary
// ray (40 %), or a bounce that leaves a point near where the primary meets the
// layer's plane, displaced by up to `hop` units per further bounce, in a
// random upward or mirrored direction. 10 % of the lanes are idle.
inline std::vector<Ray> synthetic_rays(uint32_t waves, unsigned long long seed, float layer_y = 0.2f) {
    Rng R(seed);
    std::vector<Ray> rays;
    rays.reserve((size_t)waves * 64);
    const double from[3] = {13, 2, 3};
    double w[3] = {13, 2, 3};
    const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (double &x : w) x /= wl;
    double u[3] = {w[2], 0.0, -w[0]};  // vup x w, vup = (0, 1, 0)
    const double ul = std::sqrt(u[0] * u[0] + u[2] * u[2]);
    u[0] /= ul, u[2] /= ul;
    const double v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};
    const double hh = std::tan(20.0 * M_PI / 360.0), hw = hh * 1920.0 / 1080.0;
    for (uint32_t wv = 0; wv < waves; ++wv) {
        const int tx = (int)(R.uni() * (1920 / 16)), ty = (int)(R.uni() * (1080 / 4));
        for (int l = 0; l < 64; ++l) {
            Ray r{};
            r.live = R.uni() >= 0.1;
            const double px = (16 * tx + l % 16 + R.uni()) / 1920.0, py = (4 * ty + l / 16 + R.uni()) / 1080.0;
            double d[3], o[3] = {from[0], from[1], from[2]};
            for (int k = 0; k < 3; ++k) d[k] = (2 * px - 1) * hw * u[k] + (1 - 2 * py) * hh * v[k] - w[k];
            const double seg = R.uni();
            if (seg >= 0.4 && d[1] < 0.0) {
                // where the primary meets the layer's plane, if that is near the scene
                const double t = (layer_y - o[1]) / d[1];
                double p[3] = {o[0] + t * d[0], layer_y, o[2] + t * d[2]};
                if (std::fabs(p[0]) < 14.0 && std::fabs(p[2]) < 14.0) {
                    const int bounces = seg < 0.65 ? 1 : seg < 0.85 ? 2 : 4;
                    for (int b = 1; b < bounces; ++b) p[0] += 1.5 * R.sym(), p[2] += 1.5 * R.sym();
                    o[0] = p[0], o[1] = 0.4 * R.uni(), o[2] = p[2];
                    if (R.uni() < 0.3) {  // mirrored
                        d[1] = -d[1];
                    } else {  // diffuse: upward, often shallow
                        double n;
                        do {
                            d[0] = R.sym(), d[1] = R.uni(), d[2] = R.sym();
                            n = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
                        } while (n > 1.0 || n < 1e-6);
                        if (R.uni() < 0.15) d[1] = -d[1];  // leaving a sphere's underside
                    }
                }
            }
            for (int k = 0; k < 3; ++k) r.o[k] = (float)o[k], r.d[k] = (float)d[k];
            rays.push_back(r);
        }
    }
    return rays;
}

struct Count {
    double per_ray = 0.0;   // mean marked flat blocks of a live ray
    double per_wave = 0.0;  // mean marked flat blocks of a wave's union
    uint32_t nblk = 0;      // flat blocks of the order
    long rays = 0, waves = 0, every_block = 0;  // every_block: waves some lane of which gave up
};

// rays: whole waves of 64. cell k of grid G: bit j = flat block j of nblk.
inline Count count_blocks(const rtx::LayerGrid &G, const std::vector<unsigned long long> &cell, uint32_t nblk,
                          const std::vector<Ray> &rays) {
    Count c;
    c.nblk = nblk;
    auto cellf = [&cell](uint32_t k) { return (uint64_t)cell[k]; };
    const uint64_t all = nblk >= 64 ? ~0ull : (1ull << nblk) - 1ull;
    for (size_t w = 0; w + 64 <= rays.size(); w += 64) {
        uint64_t un = 0ull;
        bool live_any = false, gave_up = false;
        for (int l = 0; l < 64; ++l) {
            const Ray &r = rays[w + l];
            if (!r.live) continue;
            live_any = true;
            uint64_t m = rtx::grid_mask_items(G, cellf, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2]);
            if (m == ~0ull) gave_up = true;
            m &= all;
            c.per_ray += (double)__builtin_popcountll(m);
            ++c.rays;
            un |= m;
        }
        if (!live_any) continue;
        if (gave_up) un = all, ++c.every_block;
        c.per_wave += (double)__builtin_popcountll(un);
        ++c.waves;
    }
    if (c.rays) c.per_ray /= (double)c.rays;
    if (c.waves) c.per_wave /= (double)c.waves;
    return c;
}

// The count for the layer of scene sph[4 n] in the given order (a scene
// without a layout or a grid: nblk = 0).
inline Count count_order(const float *sph, uint32_t n, rtx::LayoutOrder order, uint32_t tx, uint32_t tz,
                         const std::vector<Ray> &rays) {
    const rtx::SceneLayout L = rtx::build_scene_layout(sph, n, order, tx, tz);
    if (!L.valid || !L.has_grid) return Count();
    return count_blocks(L.grid, L.cell, L.flat_hi - L.flat_lo, rays);
}

}  // namespace lb
