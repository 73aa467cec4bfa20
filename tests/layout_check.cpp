// layout_check.cpp — CPU check of the small-scene spatial layout
// (raytrace-we-gpu_amd/csrc/rtx_layout.h) with the header's own code.
//
// Scenes: the RTIOW worlds of half extent 11 and 5 (the project's generator);
// random layers whose spheres are interleaved with off-layer ones in scene
// order, with layer sizes 15, 16, 8k + 3, 512 and 513; two layers of equal
// size; a scene with no layer. For every order (median split, tiles, scene):
//   - perm covers every sphere exactly once and a pad is a copy of its
//     section's last sphere; the off-layer section is in scene order;
//   - the block array holds the spheres' own floats and prefilter_R, and
//     every flat block is flat, bit for bit, at the layer's height;
//   - the layer is the largest set of bit-identical heights (ties: the one
//     whose first sphere comes first); sizes outside 16..512 give no layout;
//   - the grid over position blocks never leaves out the block of a sphere
//     the reference accepts — the adversarial ray families of grid_check.cpp
//     (near-tangent at every slope down to grazing, through cell corners,
//     along the axes, leaving a sphere's surface) with its rtx_prefilter.h
//     reference, through the DDA and through the items the kernel's wave runs;
//   - on RTIOW ext 11, with the seeded ray family of tools/layout_blocks.h, the
//     mean union of marked blocks per emulated wave is strictly below scene
//     order's (the ratio is printed, not a pass mark).
// Hostile mode (argv[3] = k > 0): the same checks again on degenerate versions
// of the RTIOW worlds and of one interleaved scene per layer size (a quarter
// of the spheres with radius 0, -0, negated, 1e-30, concentric with their
// predecessor or on the 1/8 lattice; heights kept, so the layer is the same
// set), and every k-th ray of every scene becomes the next hostile class of
// tests/hostile_rays.h. A ray outside the line test's safe range, which the
// kernel never walks, still goes through both walks (hostile_walked).
// Prints one JSON line; exit status 1 on any failure.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma layout_check.cpp ../raytrace-we-gpu_amd/csrc/rtx_host.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rtx.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_layout.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_prefilter.h"
#include "../tools/layout_blocks.h"
#include "hostile_rays.h"

static unsigned long long g_s = 0x2545f4914f6cdd1dull;
static double uni() {
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return (double)(g_s >> 11) * (1.0 / 9007199254740992.0);
}
static double sym() { return 2.0 * uni() - 1.0; }
static void unit(double v[3]) {
    do {
        v[0] = sym(), v[1] = sym(), v[2] = sym();
    } while (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] < 1e-6);
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= n, v[1] /= n, v[2] /= n;
}

static long g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_fail < 10) {                \
                fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");        \
            }                                 \
            ++g_fail;                         \
        }                                     \
    } while (0)

// hit_world32's acceptance of one sphere (best = +inf): a root >= t_min
// (grid_check.cpp's reference, the op order of oracle/rtx_oracle.c).
static bool ref_accepts(const float o[3], const float d[3], const float *c, float a, float t_min) {
    const float negr2 = -(c[3] * c[3]);
    const float ocx = o[0] - c[0], ocy = o[1] - c[1], ocz = o[2] - c[2];
    const float hb = fmaf(ocz, d[2], fmaf(ocy, d[1], ocx * d[0]));
    const float cc = fmaf(ocz, ocz, fmaf(ocy, ocy, fmaf(ocx, ocx, negr2)));
    const float disc = fmaf(hb, hb, -(a * cc));
    if (disc < 0.0f) return false;
    const float inv_a = 1.0f / a, sq = std::sqrt(disc);
    const float rn = (-hb - sq) * inv_a;
    if (!(rn < t_min || INFINITY < rn)) return true;
    const float rf = (-hb + sq) * inv_a;
    return !(rf < t_min || INFINITY < rf);
}

typedef std::vector<float> Scene;  // (cx, cy, cz, r) per sphere

static Scene rtiow(int ext) {
    const uint32_t cap = 4u * (uint32_t)(2 * ext + 1) * (uint32_t)(2 * ext + 1) + 16u;
    Scene s(4 * (size_t)cap);
    std::vector<float> mt(cap), mv(4 * (size_t)cap);
    uint32_t count = 0;
    if (rtx_scene_random_world(ext, cap, s.data(), mt.data(), mv.data(), &count) != 0) exit(2);
    s.resize(4 * (size_t)count);
    return s;
}

// `layer` spheres at height y0 interleaved at random with `off` spheres at
// other heights (each its own, so that no second layer forms).
static Scene interleaved(uint32_t layer, uint32_t off, float y0, double ext) {
    Scene s;
    uint32_t l = 0, o = 0;
    const double rmax = std::pow(10.0, -1.5 + 1.5 * uni());
    while (l < layer || o < off) {
        const bool take_layer = l < layer && (o >= off || uni() * (layer - l + off - o) < (layer - l));
        const float r = (float)(rmax * (0.05 + 0.95 * uni()));
        if (take_layer) {
            s.insert(s.end(), {(float)(ext * sym()), y0, (float)(ext * sym()), r});
            ++l;
        } else {
            // distinct heights: y0 + 1 + o / 1024 is exact and never y0
            s.insert(s.end(), {(float)(ext * sym()), y0 + 1.0f + (float)o / 1024.0f, (float)(ext * sym()), r});
            ++o;
        }
    }
    return s;
}

static long g_layouts = 0, g_rays = 0, g_accepted = 0, g_missed = 0;
static long g_hostile_every = 0, g_hostile_rays = 0, g_hostile_walked = 0, g_hostile_gave_up = 0;
static int g_hostile_cls = 0;

static Scene degenerate(Scene s) {
    for (uint32_t j = 1; j < (uint32_t)(s.size() / 4); ++j)
        if (uni() < 0.25) hostile::degenerate_sphere(s.data(), j, (int)(uni() * 6.0), true);
    return s;
}

// The structure of a layout of scene s; want_layer: the expected layer size
// (0: no layout expected), want_y: its height.
static void check_structure(const Scene &s, const rtx::SceneLayout &L, uint32_t want_layer, float want_y,
                            const char *what) {
    const uint32_t n = (uint32_t)(s.size() / 4);
    if (want_layer == 0) {
        CHECK(!L.valid, "%s: a layout where none is expected", what);
        return;
    }
    CHECK(L.valid, "%s: no layout", what);
    if (!L.valid) return;
    ++g_layouts;
    CHECK(L.n_layer == want_layer, "%s: layer of %u, expected %u", what, L.n_layer, want_layer);
    CHECK(rtx::layout_bits(L.flat_cy) == rtx::layout_bits(want_y), "%s: layer height %g, expected %g", what,
          L.flat_cy, want_y);
    const uint32_t np = (uint32_t)L.perm.size();
    CHECK(np % 8 == 0 && L.pre.size() == 4 * (size_t)np && L.flat_hi == np / 8 && L.flat_lo <= L.flat_hi,
          "%s: sizes", what);
    CHECK(np <= n + 14 && (np <= 1032 || n > 1024), "%s: %u positions for %u spheres", what, np, n);
    const uint32_t noff = n - want_layer;
    CHECK(L.flat_lo == (noff + 7) / 8 && L.flat_hi - L.flat_lo == (want_layer + 7) / 8, "%s: flat range [%u, %u)", what,
          L.flat_lo, L.flat_hi);
    // coverage: the first noff positions are the off-layer spheres in scene
    // order, then pads; the layer section holds each layer sphere once, then pads
    std::vector<uint32_t> seen(n, 0);
    uint32_t prev = 0;
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t i = L.perm[p];
        CHECK(i < n, "%s: perm[%u] = %u out of range", what, p, i);
        if (i >= n) return;
        const bool in_flat = p >= 8 * L.flat_lo;
        const uint32_t sec_lo = in_flat ? 8 * L.flat_lo : 0, sec_n = in_flat ? want_layer : noff;
        const bool pad = p >= sec_lo + sec_n;
        if (pad) {
            CHECK(i == L.perm[sec_lo + sec_n - 1], "%s: pad %u is not a copy of its section's last sphere", what, p);
        } else {
            ++seen[i];
            if (!in_flat) {
                CHECK(p == 0 || i > prev, "%s: off-layer section out of scene order at %u", what, p);
                prev = i;
            }
        }
        const bool on_layer = rtx::layout_bits(s[4 * (size_t)i + 1]) == rtx::layout_bits(want_y);
        CHECK(on_layer == in_flat, "%s: position %u (sphere %u) in the wrong section", what, p, i);
        // the block array: the sphere's floats and R
        const float *blk = &L.pre[32 * (size_t)(p / 8)];
        const float *c = &s[4 * (size_t)i];
        const float R = pad ? -INFINITY : rtx::prefilter_R(c[0], c[1], c[2], c[3] * c[3]);  // a pad is never flagged
        CHECK(rtx::layout_bits(blk[p % 8]) == rtx::layout_bits(c[0]) &&
                  rtx::layout_bits(blk[8 + p % 8]) == rtx::layout_bits(c[1]) &&
                  rtx::layout_bits(blk[16 + p % 8]) == rtx::layout_bits(c[2]) &&
                  rtx::layout_bits(blk[24 + p % 8]) == rtx::layout_bits(R),
              "%s: block floats of position %u", what, p);
        if (in_flat)
            CHECK(rtx::layout_bits(blk[8 + p % 8]) == rtx::layout_bits(L.flat_cy), "%s: flat block %u is not flat", what,
                  p / 8);
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "%s: sphere %u at %u positions", what, i, seen[i]);
}

// The grid over position blocks against the reference, on grid_check.cpp's
// ray families aimed at the layer's spheres.
static void check_grid(const Scene &s, const rtx::SceneLayout &L, long nrays, const char *what) {
    if (!L.valid || !L.has_grid) return;
    const uint32_t p_lo = 8 * L.flat_lo, np = (uint32_t)L.perm.size(), m = np - p_lo;
    const float y0 = L.flat_cy;
    auto cellf = [&L](uint32_t k) { return (uint64_t)L.cell[k]; };
    CHECK(L.grid.nblk == L.flat_hi - L.flat_lo && L.cell.size() == (size_t)L.grid.nx * L.grid.nz, "%s: grid shape", what);
    for (long k = 0; k < nrays; ++k) {
        const float *c = &s[4 * (size_t)L.perm[p_lo + (uint32_t)(uni() * m)]];
        const double r = c[3];
        double dir[3], o[3];
        const int kind = (int)(uni() * 5.0);
        unit(dir);
        if (uni() < 0.4) dir[1] = std::pow(10.0, -7.0 + 6.0 * uni()) * sym();  // grazing the layer
        if (kind == 3) {  // along an axis or level
            const int z = (int)(uni() * 3.0);
            dir[z == 0 ? 0 : z == 1 ? 2 : 1] = 0.0;
        }
        if (kind == 1) {  // aimed at a cell corner / edge
            const double cxg = L.grid.x0 + L.grid.h * std::floor(uni() * L.grid.nx);
            const double czg = L.grid.z0 + L.grid.h * std::floor(uni() * L.grid.nz);
            const double tgt[3] = {cxg + (uni() < 0.5 ? 0.0 : L.grid.h * uni()), y0 + r * sym(),
                                   czg + (uni() < 0.5 ? 0.0 : L.grid.h * uni())};
            const double back = std::pow(10.0, -1.0 + 2.5 * uni());
            for (int i = 0; i < 3; ++i) o[i] = tgt[i] - back * dir[i];
        } else if (kind == 4) {  // leaving a sphere's surface
            double nrm[3];
            unit(nrm);
            const double dl = uni() < 0.3 ? 0.0 : std::pow(10.0, -7.0 + 5.0 * uni()) * sym();
            for (int i = 0; i < 3; ++i) o[i] = c[i] + r * (1.0 + dl) * nrm[i];
            if (uni() < 0.5)
                for (int i = 0; i < 3; ++i) dir[i] = nrm[i];
        } else {  // near-tangent to sphere c
            double t[3], e[3];
            unit(t);
            const double td = t[0] * dir[0] + t[1] * dir[1] + t[2] * dir[2];
            for (int i = 0; i < 3; ++i) e[i] = t[i] - td * dir[i];
            const double en = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            if (en < 1e-9) continue;
            const double delta = std::pow(10.0, -9.0 + 8.0 * uni()) * (uni() < 0.5 ? -1.0 : 1.0);
            const double dist = uni() < 0.8 ? r * (1.0 + delta) : 2.0 * r * uni();
            const double along = sym() * std::pow(10.0, -1.0 + 2.8 * uni());
            for (int i = 0; i < 3; ++i) o[i] = c[i] + dist * e[i] / en - along * dir[i];
        }
        if (std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) > 63.9) continue;
        const double dlen = std::pow(10.0, -2.0 + 4.0 * uni());
        float of[3], df[3];
        for (int i = 0; i < 3; ++i) of[i] = (float)o[i], df[i] = (float)(dir[i] * dlen);
        const bool hz = g_hostile_every > 0 && k % g_hostile_every == 0;
        if (hz) {
            hostile::hostile_ray(g_hostile_cls++, c, of, df);
            ++g_hostile_rays;
        }
        const float a = fmaf(df[2], df[2], fmaf(df[1], df[1], df[0] * df[0]));
        const rtx::LineTest T = rtx::line_test_setup(of[0], of[1], of[2], df[0], df[1], df[2], a, 200.0f);
        if (T.thr == -INFINITY) {  // the kernel applies the grid only where the line test is safe
            if (hz) {  // the walks must still end, inside the grid
                ++g_hostile_walked;
                g_hostile_gave_up += rtx::grid_mask(L.grid, cellf, of[0], of[1], of[2], df[0], df[1], df[2]) == ~0ull;
                g_hostile_gave_up += rtx::grid_mask_items(L.grid, cellf, of[0], of[1], of[2], df[0], df[1], df[2]) == ~0ull;
            }
            continue;
        }
        ++g_rays;
        const uint64_t md = rtx::grid_mask(L.grid, cellf, of[0], of[1], of[2], df[0], df[1], df[2]);
        const uint64_t mi = rtx::grid_mask_items(L.grid, cellf, of[0], of[1], of[2], df[0], df[1], df[2]);
        for (uint32_t j = 0; j < m; ++j) {
            const float *ci = &s[4 * (size_t)L.perm[p_lo + j]];
            if (!ref_accepts(of, df, ci, a, 0.0f) && !ref_accepts(of, df, ci, a, 1e-3f)) continue;
            ++g_accepted;
            if (!((md >> (j / 8)) & 1ull) || !((mi >> (j / 8)) & 1ull)) {
                if (g_missed < 5)
                    fprintf(stderr, "%s: miss: position %u (sphere %u) o (%.9g %.9g %.9g) d (%.9g %.9g %.9g)\n", what,
                            p_lo + j, L.perm[p_lo + j], of[0], of[1], of[2], df[0], df[1], df[2]);
                ++g_missed;
            }
        }
    }
}

static void check_scene(const Scene &s, uint32_t want_layer, float want_y, long nrays, const char *what) {
    const uint32_t n = (uint32_t)(s.size() / 4);
    const struct {
        rtx::LayoutOrder order;
        uint32_t tx, tz;
    } orders[] = {{rtx::kLayoutMedian, 0, 0}, {rtx::kLayoutTiles, 4, 2}, {rtx::kLayoutTiles, 3, 3}, {rtx::kLayoutScene, 0, 0}};
    for (const auto &od : orders) {
        const rtx::SceneLayout L = rtx::build_scene_layout(s.data(), n, od.order, od.tx, od.tz);
        check_structure(s, L, want_layer, want_y, what);
        check_grid(s, L, nrays, what);
    }
}

int main(int argc, char **argv) {
    const long nrays = argc > 1 ? atol(argv[1]) : 3000;
    const uint32_t waves = argc > 2 ? (uint32_t)atol(argv[2]) : 2000;
    g_hostile_every = argc > 3 ? atol(argv[3]) : 0;
    // RTIOW: the layer is every small sphere (y = 0.2), the 4 fixed ones are off it
    const Scene w11 = rtiow(11), w5 = rtiow(5);
    check_scene(w11, (uint32_t)(w11.size() / 4) - 4, 0.2f, 4 * nrays, "rtiow11");
    check_scene(w5, (uint32_t)(w5.size() / 4) - 4, 0.2f, 4 * nrays, "rtiow5");
    // interleaved random layers: the sizes at the limits and 8k + 3
    const uint32_t sizes[] = {15, 16, 19, 67, 259, 512, 513};
    for (uint32_t ls : sizes)
        for (int rep = 0; rep < 3; ++rep) {
            const uint32_t off = rep == 0 ? 0u : 1u + (uint32_t)(uni() * 40.0);
            const float y0 = (float)(5.0 * sym());
            const double ext = std::pow(10.0, 2.5 * uni() - 1.0) * std::sqrt((double)ls);
            const Scene s = interleaved(ls, off, y0, std::fmin(ext, 40.0));
            const bool has = ls >= rtx::kLayoutMinLayer && ls <= rtx::kLayoutMaxLayer;
            char what[64];
            snprintf(what, sizeof what, "layer%u+%u", ls, off);
            check_scene(s, has ? ls : 0u, y0, nrays, what);
            if (g_hostile_every > 0 && rep == 1) {
                snprintf(what, sizeof what, "layer%u+%u degenerate", ls, off);
                check_scene(degenerate(s), has ? ls : 0u, y0, nrays, what);
            }
        }
    if (g_hostile_every > 0) {
        check_scene(degenerate(w11), (uint32_t)(w11.size() / 4) - 4, 0.2f, 4 * nrays, "rtiow11 degenerate");
        check_scene(degenerate(w5), (uint32_t)(w5.size() / 4) - 4, 0.2f, 4 * nrays, "rtiow5 degenerate");
    }
    {  // two layers of equal size: the one whose first sphere comes first
        Scene s;
        for (int i = 0; i < 48; ++i) s.insert(s.end(), {(float)(8.0 * sym()), i % 2 ? 1.5f : -0.25f, (float)(8.0 * sym()), 0.3f});
        check_scene(s, 24, -0.25f, nrays, "two_layers");
        Scene t;  // ... whichever height is the larger number
        for (int i = 0; i < 48; ++i) t.insert(t.end(), {(float)(8.0 * sym()), i % 2 ? -0.25f : 1.5f, (float)(8.0 * sym()), 0.3f});
        check_scene(t, 24, 1.5f, nrays, "two_layers_swapped");
        Scene z;  // +0 and -0 are different layers
        for (int i = 0; i < 40; ++i) z.insert(z.end(), {(float)(8.0 * sym()), i < 18 ? 0.0f : -0.0f, (float)(8.0 * sym()), 0.3f});
        check_scene(z, 22, -0.0f, nrays, "signed_zero");
    }
    {  // no layer: every height its own
        Scene s;
        for (int i = 0; i < 100; ++i) s.insert(s.end(), {(float)(8.0 * sym()), (float)i / 64.0f, (float)(8.0 * sym()), 0.3f});
        check_scene(s, 0, 0.0f, nrays, "no_layer");
        check_scene(Scene(), 0, 0.0f, nrays, "empty");
    }
    // the point of it: fewer marked blocks per wave than scene order, RTIOW ext 11
    const std::vector<lb::Ray> rays = lb::synthetic_rays(waves, 1);
    const uint32_t n11 = (uint32_t)(w11.size() / 4);
    const lb::Count cs = lb::count_order(w11.data(), n11, rtx::kLayoutScene, 0, 0, rays);
    const lb::Count cm = lb::count_order(w11.data(), n11, rtx::kLayoutDefault, 4, 2, rays);
    CHECK(cs.waves > 0 && cm.waves == cs.waves && cm.nblk == cs.nblk, "block counts: waves");
    CHECK(cm.per_wave < cs.per_wave, "default order marks %.3f blocks per wave, scene order %.3f", cm.per_wave,
          cs.per_wave);
    CHECK(g_missed == 0, "%ld accepted spheres missing from the grid", g_missed);
    printf("{\"layouts\": %ld, \"rays\": %ld, \"accepted_spheres\": %ld, \"missed\": %ld, \"failures\": %ld, "
           "\"scene_blocks_per_wave\": %.3f, \"layout_blocks_per_wave\": %.3f, \"ratio\": %.3f, "
           "\"scene_blocks_per_ray\": %.3f, \"layout_blocks_per_ray\": %.3f, \"hostile_rays\": %ld, "
           "\"hostile_walked\": %ld, \"hostile_gave_up\": %ld}\n",
           g_layouts, g_rays, g_accepted, g_missed, g_fail, cs.per_wave, cm.per_wave,
           cs.per_wave > 0.0 ? cm.per_wave / cs.per_wave : 0.0, cs.per_ray, cm.per_ray, g_hostile_rays,
           g_hostile_walked, g_hostile_gave_up);
    return g_fail == 0 ? 0 : 1;
}
