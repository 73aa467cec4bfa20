// regime_check.cpp — which branches of the layer-grid walk a set of rays
// reaches on a small scene, with the headers' own code (rtx_layout.h,
// rtx_grid.h). tests/test_scan_regimes.py feeds it the pixel-centre primary
// rays of every (world, camera) of tests/regime_cases.py: the frame tests of
// test_gpu_scan_regimes.py are only worth their name if those rays do take
// the walks they are meant for.
//
// Input (argv[1]), little endian: uint32 n, uint32 nrays, uint32 use_layout,
// uint32 0; n * 4 floats (cx, cy, cz, r); nrays * 6 floats (origin,
// direction). use_layout: whether rtx_upload_world keeps the scene's layout
// (it drops a valid one that does not fit the render's LDS beside the sphere
// copy, rtx_kernels.hip layout_lds_ok: device-side knowledge the caller has
// from the regime table). The grid is then the layout's, over position
// blocks, or the one over the scene-order flat run, found and built as
// rtx_upload_world does.
// Each ray is classified by grid_stretch (what a lane of grid_wave_mask
// computes): gave up because |o| > kGridOMax; gave up otherwise (more than
// kGridMaxSteps columns, no end, a slope that is not a number); never enters
// the slab inside the grid; 1-4, 5-16 or 17-48 items. The items' cells are
// read as the wave reads them (grid_item_cells) and must name a block of the
// run for every ray that has items.
// Prints one JSON line; exit status 1 on a malformed input or a failed check.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma regime_check.cpp ../raytrace-we-gpu_amd/csrc/rtx_host.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_layout.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_prefilter.h"

// The longest run of flat blocks of `pre` in scene order, as rtx_upload_world
// finds it: all 8 centre heights of a block equal bit for bit (the last block
// padded with copies of sphere n - 1) and equal along the run.
static void scene_flat_run(const std::vector<float> &sph, uint32_t n, uint32_t &flat_lo, uint32_t &flat_hi,
                           float &flat_cy) {
    flat_lo = flat_hi = 0;
    flat_cy = 0.0f;
    const uint32_t nblk = (n + 7) / 8;
    auto bits = [&](uint32_t b, int k) {
        const uint32_t i = std::min(8 * b + (uint32_t)k, n - 1);
        return rtx::layout_bits(sph[4 * (size_t)i + 1]);
    };
    auto flat = [&](uint32_t b) {
        for (int k = 1; k < 8; ++k)
            if (bits(b, k) != bits(b, 0)) return false;
        return true;
    };
    for (uint32_t b = 0; b < nblk;) {
        if (!flat(b)) {
            ++b;
            continue;
        }
        uint32_t e = b + 1;
        while (e < nblk && flat(e) && bits(e, 0) == bits(b, 0)) ++e;
        if (e - b > flat_hi - flat_lo) flat_lo = b, flat_hi = e, flat_cy = sph[4 * (size_t)std::min(8 * b, n - 1) + 1];
        b = e;
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: regime_check CASE.bin\n");
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    uint32_t head[4] = {0, 0, 0, 0};
    if (fread(head, sizeof(uint32_t), 4, f) != 4 || head[0] > (1u << 20) || head[1] > (1u << 24)) {
        fprintf(stderr, "regime_check: bad header\n");
        return 1;
    }
    const uint32_t n = head[0], nrays = head[1];
    const bool use_layout = head[2] != 0;
    std::vector<float> sph(4 * (size_t)n), rays(6 * (size_t)nrays);
    if (fread(sph.data(), sizeof(float), sph.size(), f) != sph.size() ||
        fread(rays.data(), sizeof(float), rays.size(), f) != rays.size()) {
        fprintf(stderr, "regime_check: short file\n");
        return 1;
    }
    fclose(f);

    rtx::SceneLayout lay;  // (small scenes only: n_pad <= kScanPfMin of rtx_internal.h, 1,024)
    if (n != 0 && (n + 7) / 8 * 8 <= 1024) lay = rtx::build_scene_layout(sph.data(), n, rtx::kLayoutDefault);
    const bool valid = lay.valid;
    const uint32_t positions = valid ? (uint32_t)lay.perm.size() : 0;
    const uint32_t n_layer = lay.n_layer;
    uint32_t flat_lo = 0, flat_hi = 0;
    float flat_cy = 0.0f;
    bool has_grid = false;
    rtx::LayerGrid grid{};
    std::vector<unsigned long long> cell;
    if (valid && use_layout) {
        flat_lo = lay.flat_lo, flat_hi = lay.flat_hi, flat_cy = lay.flat_cy;
        has_grid = lay.has_grid;
        grid = lay.grid;
        cell.swap(lay.cell);
    } else if (n != 0) {
        scene_flat_run(sph, n, flat_lo, flat_hi, flat_cy);
        has_grid = flat_hi > flat_lo &&
                   rtx::build_layer_grid(sph.data(), 8 * flat_lo, std::min(8 * flat_hi, n), grid, cell);
    }

    long far = 0, gave_up = 0, none = 0, i1_4 = 0, i5_16 = 0, i17_48 = 0, failures = 0;
    unsigned long long marked = 0;
    if (has_grid) {
        const unsigned long long run_mask = grid.nblk >= 64 ? ~0ull : (1ull << grid.nblk) - 1ull;
        if (cell.size() != (size_t)grid.nx * grid.nz || grid.nblk != flat_hi - flat_lo) ++failures;
        for (uint32_t r = 0; r < nrays; ++r) {
            const float *q = &rays[6 * (size_t)r];
            rtx::GridStretch R;
            if (!rtx::grid_stretch(grid, q[0], q[1], q[2], q[3], q[4], q[5], R)) {
                const float o2 = fmaf(q[0], q[0], fmaf(q[1], q[1], q[2] * q[2]));
                if (!(o2 <= rtx::kGridOMax * rtx::kGridOMax))
                    ++far;
                else
                    ++gave_up;
                continue;
            }
            if (R.n == 0) {
                ++none;
                continue;
            }
            (R.n <= 4 ? i1_4 : R.n <= 16 ? i5_16 : i17_48)++;
            if (R.n > rtx::kGridMaxSteps) ++failures;
            unsigned long long m = 0;
            for (uint32_t i = 0; i < R.n; ++i) {
                uint32_t k0, stride, cnt;
                rtx::grid_item_cells(grid, R.lo, R.hi, R.A, R.s, R.zmajor, R.c0 + i, k0, stride, cnt);
                for (uint32_t c = 0; c < cnt; ++c) m |= cell.at(k0 + c * stride);
            }
            if (m & ~run_mask) ++failures;
            marked += (unsigned long long)__builtin_popcountll(m);
        }
    }
    printf("{\"n\": %u, \"rays\": %u, \"valid\": %d, \"layout\": %d, \"layout_positions\": %u, \"n_layer\": %u, "
           "\"flat_lo\": %u, \"flat_hi\": %u, \"flat_cy\": %.9g, \"grid\": %d, \"grid_nx\": %u, \"grid_nz\": %u, "
           "\"far\": %ld, \"gave_up\": %ld, \"none\": %ld, \"items_1_4\": %ld, \"items_5_16\": %ld, "
           "\"items_17_48\": %ld, \"blocks_marked\": %llu, \"failures\": %ld}\n",
           n, nrays, valid ? 1 : 0, valid && use_layout ? 1 : 0, valid && use_layout ? positions : 0, n_layer, flat_lo,
           flat_hi, (double)flat_cy, has_grid ? 1 : 0, has_grid ? grid.nx : 0, has_grid ? grid.nz : 0, far, gave_up,
           none, i1_4, i5_16, i17_48, marked, failures);
    return failures ? 1 : 0;
}
