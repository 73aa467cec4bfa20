// layout_blocks.cpp — the CPU tool that chooses the order of the layer's
// spheres (rtx_layout.h): for a scene and a set of rays it emulates waves of
// 64 rays and prints the flat blocks the layer grid marks per ray and per wave
// union, for scene order and for each candidate order. One JSON line per order.
//
//   layout_blocks [--ext N] [--scene FILE] [--rays FILE] [--waves W] [--seed S]
//
// --ext N      the RTIOW world of half extent N (default 11: the flagship's)
// --scene FILE raw float32 (cx, cy, cz, r) per sphere, instead
// --rays FILE  raw float32 records (o.xyz, d.xyz, live) per lane, 64 lanes per
//              wave: real lane-mode rays (tools/layout_blocks.py converts the
//              sample tools/ray_sample.py takes on the GPU). Without it: the
//              seeded synthetic family of layout_blocks.h.
// Build (tools/layout_blocks.py does it): g++ -O2 -std=c++17 -ffp-contract=off -mfma
//   tools/layout_blocks.cpp raytrace-we-gpu_amd/csrc/rtx_host.cpp -o layout_blocks
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rtx.h"
#include "layout_blocks.h"

static std::vector<float> read_f32(const char *path) {
    std::vector<float> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    float buf[4096];
    size_t k;
    while ((k = fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv) {
    int ext = 11;
    const char *scene = nullptr, *rays_path = nullptr;
    uint32_t waves = 4000;
    unsigned long long seed = 1;
    for (int i = 1; i < argc; ++i) {
        auto val = [&]() -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s needs a value\n", argv[i]);
                exit(2);
            }
            return argv[++i];
        };
        if (!strcmp(argv[i], "--ext")) ext = atoi(val());
        else if (!strcmp(argv[i], "--scene")) scene = val();
        else if (!strcmp(argv[i], "--rays")) rays_path = val();
        else if (!strcmp(argv[i], "--waves")) waves = (uint32_t)atol(val());
        else if (!strcmp(argv[i], "--seed")) seed = strtoull(val(), nullptr, 10);
        else {
            fprintf(stderr, "unknown argument %s\n", argv[i]);
            return 2;
        }
    }
    std::vector<float> sph;
    if (scene) {
        sph = read_f32(scene);
    } else {
        const uint32_t cap = 4u * (uint32_t)(2 * ext + 1) * (uint32_t)(2 * ext + 1) + 16u;
        sph.resize(4 * (size_t)cap);
        std::vector<float> mt(cap), mv(4 * (size_t)cap);
        uint32_t count = 0;
        if (rtx_scene_random_world(ext, cap, sph.data(), mt.data(), mv.data(), &count) != 0) return 2;
        sph.resize(4 * (size_t)count);
    }
    const uint32_t n = (uint32_t)(sph.size() / 4);
    std::vector<lb::Ray> rays;
    if (rays_path) {
        const std::vector<float> raw = read_f32(rays_path);
        for (size_t k = 0; k + 7 <= raw.size(); k += 7) {
            lb::Ray r;
            for (int j = 0; j < 3; ++j) r.o[j] = raw[k + j], r.d[j] = raw[k + 3 + j];
            r.live = raw[k + 6] != 0.0f;
            rays.push_back(r);
        }
    } else {
        const std::vector<uint32_t> layer = rtx::layout_find_layer(sph.data(), n);
        rays = lb::synthetic_rays(waves, seed, layer.empty() ? 0.2f : sph[4 * (size_t)layer[0] + 1]);
    }
    struct Cand {
        const char *name;
        rtx::LayoutOrder order;
        uint32_t tx, tz;
    };
    const Cand cands[] = {{"scene", rtx::kLayoutScene, 0, 0},   {"median", rtx::kLayoutMedian, 0, 0},
                          {"tiles3x3", rtx::kLayoutTiles, 3, 3}, {"tiles2x4", rtx::kLayoutTiles, 2, 4},
                          {"tiles4x2", rtx::kLayoutTiles, 4, 2}};
    double base = 0.0;
    for (const Cand &c : cands) {
        const lb::Count k = lb::count_order(sph.data(), n, c.order, c.tx, c.tz, rays);
        if (k.nblk == 0) {
            printf("{\"order\": \"%s\", \"layout\": false, \"spheres\": %u}\n", c.name, n);
            continue;
        }
        if (c.order == rtx::kLayoutScene) base = k.per_wave;
        printf("{\"order\": \"%s\", \"spheres\": %u, \"flat_blocks\": %u, \"rays\": \"%s\", \"waves\": %ld, "
               "\"live_rays\": %ld, \"blocks_per_ray\": %.3f, \"blocks_per_wave\": %.3f, \"vs_scene\": %.3f, "
               "\"waves_every_block\": %ld}\n",
               c.name, n, k.nblk, rays_path ? "file" : "synthetic", k.waves, k.rays, k.per_ray, k.per_wave,
               base > 0.0 ? k.per_wave / base : 0.0, k.every_block);
    }
    return 0;
}
