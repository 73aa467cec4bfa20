// walk_items_check.cpp — the item count and the block mask of every ray of a
// set on a small scene with a layout, with the headers' own code
// (rtx_layout.h build_scene_layout; rtx_grid.h grid_stretch, grid_mask_items):
// what a lane of rtx_kernels.hip grid_wave_mask computes for it. For
// tests/test_gpu_walk_prefix.py, which chooses its waves by these counts and
// checks the oracle's hits against these masks.
//
// Input (argv[1]), little endian, as regime_check.cpp's: uint32 n, uint32
// nrays, uint32 0, uint32 0; n * 4 floats (cx, cy, cz, r); nrays * 6 floats
// (origin, direction). The scene must have a layout with a grid.
// Output (argv[2]): uint32 flat_lo, flat_hi, positions, nrays; uint32
// perm[positions] (position -> scene index); int32 items[nrays] (-1: the lane
// gives up and the wave scans every block); uint64 mask[nrays] (bit j: block
// flat_lo + j; ~0 for a lane that gives up).
// Exit status 1 on a malformed input, a scene without such a grid, or a ray
// whose count passes kGridMaxSteps.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma walk_items_check.cpp ../raytrace-we-gpu_amd/csrc/rtx_host.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_layout.h"

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: walk_items_check CASE.bin OUT.bin\n");
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    uint32_t head[4] = {0, 0, 0, 0};
    if (fread(head, sizeof(uint32_t), 4, f) != 4 || head[0] == 0 || head[0] > 1024u || head[1] > (1u << 24)) {
        fprintf(stderr, "walk_items_check: bad header\n");
        return 1;
    }
    const uint32_t n = head[0], nrays = head[1];
    std::vector<float> sph(4 * (size_t)n), rays(6 * (size_t)nrays);
    if (fread(sph.data(), sizeof(float), sph.size(), f) != sph.size() ||
        fread(rays.data(), sizeof(float), rays.size(), f) != rays.size()) {
        fprintf(stderr, "walk_items_check: short file\n");
        return 1;
    }
    fclose(f);
    const rtx::SceneLayout lay = rtx::build_scene_layout(sph.data(), n, rtx::kLayoutDefault);
    if (!lay.valid || !lay.has_grid || lay.grid.nblk != lay.flat_hi - lay.flat_lo) {
        fprintf(stderr, "walk_items_check: the scene has no layout with a grid\n");
        return 1;
    }
    auto cell = [&lay](uint32_t k) { return (uint64_t)lay.cell.at(k); };
    std::vector<int32_t> items(nrays);
    std::vector<uint64_t> mask(nrays);
    int bad = 0;
    for (uint32_t r = 0; r < nrays; ++r) {
        const float *q = &rays[6 * (size_t)r];
        rtx::GridStretch R;
        const bool ok = rtx::grid_stretch(lay.grid, q[0], q[1], q[2], q[3], q[4], q[5], R);
        items[r] = ok ? (int32_t)R.n : -1;
        if (ok && R.n > rtx::kGridMaxSteps) ++bad;
        mask[r] = rtx::grid_mask_items(lay.grid, cell, q[0], q[1], q[2], q[3], q[4], q[5]);
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) {
        perror(argv[2]);
        return 1;
    }
    const uint32_t out[4] = {lay.flat_lo, lay.flat_hi, (uint32_t)lay.perm.size(), nrays};
    fwrite(out, sizeof(uint32_t), 4, g);
    fwrite(lay.perm.data(), sizeof(uint32_t), lay.perm.size(), g);
    fwrite(items.data(), sizeof(int32_t), items.size(), g);
    fwrite(mask.data(), sizeof(uint64_t), mask.size(), g);
    fclose(g);
    printf("{\"rays\": %u, \"grid_nx\": %u, \"grid_nz\": %u, \"max_items\": %u, \"bad\": %d}\n", nrays, lay.grid.nx,
           lay.grid.nz, rtx::kGridMaxSteps, bad);
    return bad ? 1 : 0;
}
