// setup_equiv_check.cpp — the straight-line segment set-up against the
// early-return form it replaced.
//
// grid_stretch (rtx_grid.h) computes all its outputs for every ray and decides
// the outcome once at the end. The form it replaced, with its nested early
// returns, is kept below verbatim (namespace spec) as the specification, and
// so is line_test_setup (rtx_prefilter.h), which runs before it in every
// segment's set-up and keeps its early return (its straight-line form was
// tried and not kept, RESULTS.md S13; the copy pins its values):
//   * grid_stretch: the same return value (gives up or not) and the same n for
//     every ray; for a ray with items (n > 0) all seven outputs are the same
//     bits. A ray that gives up or never enters the slab has n = 0 in both and
//     nothing else of it is read (grid_wave_mask, grid_mask_items): the other
//     outputs of the new form are not compared there;
//   * grid_mask_items over the new grid_stretch equals the same loop over the
//     specification's, for every ray;
//   * line_test_setup: all eight outputs are the same bits for every ray, safe
//     or not, at every setting of the host's rsq / sqrt ulp model, for the ray
//     as it is and stretched along y (line_test_stretched's inputs).
// Rays: the layers and adversarial families of grid_check.cpp /
// grid_coop_check.cpp (near-tangent at every slope down to grazing, through
// cell corners and edges, along the axes or level with components exactly +0
// and -0, leaving a sphere's surface, origins on the slab's and the box's
// faces), dy = 0 inside the slab, |o| a few ulps below and above kGridOMax,
// and every hostile class of hostile_rays.h (NaN, infinite, zero, tiny and
// huge components). Every outcome must occur often enough (min_each).
// Prints one JSON line; exit status 1 on a difference or a starved outcome.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma setup_equiv_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_prefilter.h"
#include "hostile_rays.h"

namespace spec {
using namespace rtx;

// rtx_prefilter.h line_test_setup (host build)
static inline LineTest line_test_setup(float ox, float oy, float oz, float dx, float dy, float dz, float a,
                                       float smag) {
    LineTest T;
    const float m2 = fmaf(dy, dy, dz * dz);
    const float o2 = fmaf(ox, ox, fmaf(oy, oy, oz * oz));
    const float so = smag + pf_sqrt(o2);
    const float so2 = so * so;
    const bool safe = a >= 9.094947e-13f && a <= 1.0995116e12f && m2 >= a * 9.094947e-13f &&
                      so2 <= 1e36f && a * so2 <= 1e36f;
    if (!safe) {
        T.ux = T.uy = T.uz = T.vy = T.vz = T.nou = T.nov = 0.0f;
        T.thr = -INFINITY;
        return T;
    }
    const float inv_m = pf_rsq_k(m2, 0);
    const float w = pf_rsq_k(a, 1) * inv_m;
    T.vy = dz * inv_m;
    T.vz = -dy * inv_m;
    T.ux = -(m2 * w);
    T.uy = (dx * dy) * w;
    T.uz = (dx * dz) * w;
    T.nou = -fmaf(oz, T.uz, fmaf(oy, T.uy, ox * T.ux));
    T.nov = -fmaf(oz, T.vz, oy * T.vy);
    T.thr = -fmaf(o2, kPreMarginO, kPreFloor);
    return T;
}

// rtx_grid.h grid_stretch before the straight-line form
static inline bool grid_stretch(const LayerGrid &G, float ox, float oy, float oz, float dx, float dy, float dz,
                                GridStretch &R) {
    R.lo = R.hi = R.A = R.s = 0.0f;
    R.c0 = R.n = R.zmajor = 0u;
    const float o2 = fmaf(ox, ox, fmaf(oy, oy, oz * oz));
    const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
    if (!(o2 <= kGridOMax * kGridOMax) || !(d2 <= 3.0e38f)) return false;  // far or non-finite
    const float inf = INFINITY;
    float t0 = 0.0f, t1 = inf;
    // grid_walk's clips, op for op (the same t0, t1); returns 1 / d (0 for d = 0)
    auto clip = [&](float o, float d, float lo, float hi) {
        if (d == 0.0f) {
            if (!(o >= lo && o <= hi)) t1 = -inf;
            return 0.0f;
        }
        const float inv = 1.0f / d;
        const float ta = (lo - o) * inv, tb = (hi - o) * inv;
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
        return inv;
    };
    clip(oy, dy, G.ylo, G.yhi);
    const float ivx = clip(ox, dx, G.x0, G.x0 + (float)G.nx * G.h);
    const float ivz = clip(oz, dz, G.z0, G.z0 + (float)G.nz * G.h);
    if (!(t0 <= t1)) return true;
    if (!(t1 <= 3.0e38f)) return false;  // no end: d = 0 along x and z, or overflow
    const bool zm = fabsf(dz) > fabsf(dx);
    const float om = zm ? oz : ox, dm = zm ? dz : dx, on = zm ? ox : oz, dn = zm ? dx : dz;
    const float M0 = zm ? G.z0 : G.x0, N0 = zm ? G.x0 : G.z0;
    const float nM = (float)(zm ? G.nz : G.nx);
    const float s = dn * (zm ? ivz : ivx);  // |dn| <= |dm|: |s| <= 1 + 2u, or 0 (dm = 0), or not a number (1 / dm overflowed)
    if (!(fabsf(s) <= 2.0f)) return false;
    const float a0 = (fmaf(t0, dm, om) - M0) * G.inv_h, a1 = (fmaf(t1, dm, om) - M0) * G.inv_h;
    const float b0 = (fmaf(t0, dn, on) - N0) * G.inv_h;
    R.lo = fminf(a0, a1), R.hi = fmaxf(a0, a1);
    R.s = s;
    R.A = fmaf(-a0, s, b0);
    const float c0 = grid_clampf(floorf(R.lo - kGridCoopEps), 0.0f, nM - 1.0f);
    const float c1 = grid_clampf(floorf(R.hi + kGridCoopEps), 0.0f, nM - 1.0f);
    R.c0 = (uint32_t)c0;
    R.zmajor = zm ? 1u : 0u;
    const uint32_t n = (uint32_t)c1 - (uint32_t)c0 + 1u;
    if (n > kGridMaxSteps) return false;
    R.n = n;
    return true;
}

// rtx_grid.h grid_mask_items over the specification's grid_stretch
template <typename Cell>
static inline uint64_t grid_mask_items(const LayerGrid &G, Cell cell, float ox, float oy, float oz, float dx, float dy,
                                       float dz) {
    GridStretch R;
    if (!spec::grid_stretch(G, ox, oy, oz, dx, dy, dz, R)) return ~0ull;
    uint64_t m = 0ull;
    for (uint32_t i = 0; i < R.n; ++i) {
        uint32_t k0, stride, cnt;
        grid_item_cells(G, R.lo, R.hi, R.A, R.s, R.zmajor, R.c0 + i, k0, stride, cnt);
        for (uint32_t q = 0; q < cnt; ++q) m |= cell(k0 + q * stride);
    }
    return m;
}
}  // namespace spec

static unsigned long long g_s = 0x9e3779b97f4a7c15ull;
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

struct Layer {
    std::vector<float> s;  // (cx, cy, cz, r)
    rtx::LayerGrid G;
    std::vector<unsigned long long> cell;
};
struct Ray {
    float o[3], d[3];
};

// the layers of grid_coop_check.cpp
static bool make_layer(Layer &L, bool rtiow) {
    L.s.clear();
    if (rtiow) {  // the layer of random_world(11): unit cells, jitter 0.9, r 0.2
        for (int a = -11; a < 11; ++a)
            for (int b = -11; b < 11; ++b) {
                if (uni() < 0.03) continue;
                L.s.insert(L.s.end(), {(float)(a + 0.9 * uni()), 0.2f, (float)(b + 0.9 * uni()), 0.2f});
                if (L.s.size() / 4 == 480) break;
            }
    } else {
        const int n = 8 + (int)(uni() * 505);
        const float y0 = (float)(5.0 * sym());
        const double ext = std::pow(10.0, 4.0 * uni() - 2.0) * std::sqrt((double)n);
        const double rmax = std::pow(10.0, -2.0 + 2.3 * uni());
        for (int i = 0; i < n; ++i)
            L.s.insert(L.s.end(), {(float)(ext * sym()), y0, (float)(ext * sym()), (float)(rmax * (0.05 + 0.95 * uni()))});
    }
    return rtx::build_layer_grid(L.s.data(), 0u, (uint32_t)(L.s.size() / 4), L.G, L.cell);
}

// One ray of the layer: grid_coop_check.cpp's families (kinds 0-6) and this
// check's own (7: dy = 0 inside the slab, 8: |o| at kGridOMax, 9: signed
// zeros); false when the draw is dropped.
static bool make_ray(const Layer &L, Ray &R) {
    const uint32_t n = (uint32_t)(L.s.size() / 4);
    const float *c = &L.s[4 * (size_t)(uni() * n)];
    const float y0 = L.s[1];
    const double r = c[3];
    double dir[3], o[3];
    const int kind = (int)(uni() * 10.0);
    unit(dir);
    if (uni() < 0.4) dir[1] = std::pow(10.0, -7.0 + 6.0 * uni()) * sym();  // grazing the layer
    if (kind == 3) {  // along an axis or level
        const int z = (int)(uni() * 3.0);
        dir[z == 0 ? 0 : z == 1 ? 2 : 1] = 0.0;
        if (uni() < 0.3) dir[z == 0 ? 2 : 0] = 0.0;  // two components 0
    }
    const double xlo = L.G.x0, xhi = L.G.x0 + (double)L.G.nx * L.G.h, zlo = L.G.z0, zhi = L.G.z0 + (double)L.G.nz * L.G.h;
    bool keep_far = false;
    if (kind == 1) {  // aimed at a cell corner / edge, from anywhere
        const double cxg = L.G.x0 + L.G.h * std::floor(uni() * L.G.nx), czg = L.G.z0 + L.G.h * std::floor(uni() * L.G.nz);
        const double tgt[3] = {cxg + (uni() < 0.5 ? 0.0 : L.G.h * uni()), y0 + r * sym(), czg + (uni() < 0.5 ? 0.0 : L.G.h * uni())};
        const double back = std::pow(10.0, -1.0 + 2.5 * uni());
        for (int i = 0; i < 3; ++i) o[i] = tgt[i] - back * dir[i];
    } else if (kind == 4) {  // leaving a sphere's surface (radially, or at random)
        double nrm[3];
        unit(nrm);
        const double dl = uni() < 0.3 ? 0.0 : std::pow(10.0, -7.0 + 5.0 * uni()) * sym();
        for (int i = 0; i < 3; ++i) o[i] = c[i] + r * (1.0 + dl) * nrm[i];
        if (uni() < 0.5)
            for (int i = 0; i < 3; ++i) dir[i] = nrm[i];
    } else if (kind == 5) {  // origin on a face of the slab or of the box (fp32-exact), or on a cell boundary
        o[0] = xlo + (xhi - xlo) * uni(), o[1] = y0 + 3.0 * r * sym(), o[2] = zlo + (zhi - zlo) * uni();
        const int f = (int)(uni() * 7.0);
        if (f == 0) o[1] = L.G.ylo;
        if (f == 1) o[1] = L.G.yhi;
        if (f == 2) o[0] = xlo;
        if (f == 3) o[0] = xhi;
        if (f == 4) o[2] = zlo;
        if (f == 5) o[2] = zhi;
        if (f == 6) o[0] = L.G.x0 + L.G.h * std::floor(uni() * L.G.nx), o[1] = (L.G.ylo + L.G.yhi) * 0.5;
    } else if (kind == 6) {  // random: from anywhere towards the layer's box
        const double ext = std::fmax(xhi - xlo, zhi - zlo);
        for (int i = 0; i < 3; ++i) o[i] = std::fmin(ext, 36.0) * sym();
        const double tgt[3] = {xlo + (xhi - xlo) * uni(), y0, zlo + (zhi - zlo) * uni()};
        if (uni() < 0.7)
            for (int i = 0; i < 3; ++i) dir[i] = tgt[i] - o[i];
    } else if (kind == 7) {  // level (dy exactly 0, either sign), inside the slab, on its faces or outside it
        o[0] = xlo + (xhi - xlo) * (1.4 * uni() - 0.2), o[2] = zlo + (zhi - zlo) * (1.4 * uni() - 0.2);
        const int f = (int)(uni() * 5.0);
        o[1] = f == 0 ? L.G.ylo : f == 1 ? L.G.yhi : f == 2 ? y0 + 4.0 * r * sym() : L.G.ylo + (L.G.yhi - L.G.ylo) * uni();
        dir[1] = uni() < 0.5 ? 0.0 : -0.0;
        if (uni() < 0.2) dir[uni() < 0.5 ? 0 : 2] = uni() < 0.5 ? 0.0 : -0.0;
    } else if (kind == 8) {  // |o| within a few ulps of kGridOMax, aimed at the layer
        unit(o);
        const double tgt[3] = {xlo + (xhi - xlo) * uni(), y0, zlo + (zhi - zlo) * uni()};
        const double rad = (double)rtx::kGridOMax * (1.0 + 6e-8 * (double)((int)(uni() * 9.0) - 4));
        for (int i = 0; i < 3; ++i) o[i] *= rad, dir[i] = tgt[i] - o[i];
        keep_far = true;
    } else if (kind == 9) {  // components exactly +0 / -0, origin anywhere near the box
        o[0] = xlo + (xhi - xlo) * uni(), o[1] = y0 + 6.0 * r * sym(), o[2] = zlo + (zhi - zlo) * uni();
        const int z = (int)(uni() * 6.0);  // which components are zero
        for (int i = 0; i < 3; ++i)
            if ((z == i) || (z >= 3 && z - 3 != i)) dir[i] = uni() < 0.5 ? 0.0 : -0.0;
    } else {  // near-tangent to sphere c (kinds 0, 2, 3)
        double t[3], e[3];
        unit(t);
        const double td = t[0] * dir[0] + t[1] * dir[1] + t[2] * dir[2];
        for (int i = 0; i < 3; ++i) e[i] = t[i] - td * dir[i];
        const double en = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        if (en < 1e-9) return false;
        const double delta = std::pow(10.0, -9.0 + 8.0 * uni()) * (uni() < 0.5 ? -1.0 : 1.0);
        const double dist = uni() < 0.8 ? r * (1.0 + delta) : 2.0 * r * uni();
        const double along = sym() * std::pow(10.0, -1.0 + 2.8 * uni());
        for (int i = 0; i < 3; ++i) o[i] = c[i] + dist * e[i] / en - along * dir[i];
    }
    const double on = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    if (on > 63.9 && !keep_far) return false;
    const double dn = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    if (!(dn > 0.0)) return false;
    const double dlen = std::pow(10.0, -2.0 + 4.0 * uni()) / dn;
    for (int i = 0; i < 3; ++i) R.o[i] = (float)o[i], R.d[i] = (float)(dir[i] * dlen);
    return true;
}

static bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }
static bool same_line(const rtx::LineTest &a, const rtx::LineTest &b) {
    const float x[8] = {a.ux, a.uy, a.uz, a.vy, a.vz, a.nou, a.nov, a.thr};
    const float y[8] = {b.ux, b.uy, b.uz, b.vy, b.vz, b.nou, b.nov, b.thr};
    return same_bits(x, y, sizeof x);
}
static bool same_stretch(const rtx::GridStretch &a, const rtx::GridStretch &b) {
    const float x[4] = {a.lo, a.hi, a.A, a.s}, y[4] = {b.lo, b.hi, b.A, b.s};
    return same_bits(x, y, sizeof x) && a.c0 == b.c0 && a.n == b.n && a.zmajor == b.zmajor;
}

int main(int argc, char **argv) {
    const long nlayers = argc > 1 ? atol(argv[1]) : 150;
    const long nrays = argc > 2 ? atol(argv[2]) : 4000;
    const long min_each = argc > 3 ? atol(argv[3]) : 1000;
    const long hostile_every = argc > 4 ? atol(argv[4]) : 7;
    long rays = 0, layers = 0, line_bad = 0, line_safe = 0, line_unsafe = 0;
    long st_bad = 0, st_items = 0, st_none = 0, st_quit = 0, mask_bad = 0, dy0_inside = 0, near_omax = 0;
    int hostile_cls = 0;
    for (long li = 0; li < nlayers; ++li) {
        Layer L;
        if (!make_layer(L, li % 3 == 0)) continue;
        ++layers;
        auto cellf = [&L](uint32_t k) { return (uint64_t)L.cell[k]; };
        for (long k = 0; k < nrays; ++k) {
            Ray r;
            if (!make_ray(L, r)) continue;
            if (hostile_every > 0 && k % hostile_every == 0)
                hostile::hostile_ray(hostile_cls++, &L.s[4 * (size_t)(uni() * (double)(L.s.size() / 4))], r.o, r.d);
            ++rays;
            const float *o = r.o, *d = r.d;
            dy0_inside += d[1] == 0.0f && o[1] >= L.G.ylo && o[1] <= L.G.yhi;
            const float o2 = fmaf(o[0], o[0], fmaf(o[1], o[1], o[2] * o[2]));
            near_omax += std::fabs(o2 - 4096.0f) <= 0.01f;
            // the line test, as it is and stretched along y, at every ulp setting of the host's rsq / sqrt model
            const float a = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
            const float dys = rtx::kCullSy * d[1];
            const float as = fmaf(d[2], d[2], fmaf(dys, dys, d[0] * d[0]));
            for (int u = 0; u < 27; ++u) {
                rtx::pf_host_ulp[0] = u % 3 - 1, rtx::pf_host_ulp[1] = (u / 3) % 3 - 1, rtx::pf_host_ulp[2] = u / 9 - 1;
                const rtx::LineTest T = rtx::line_test_setup(o[0], o[1], o[2], d[0], d[1], d[2], a, 200.0f);
                const rtx::LineTest W = spec::line_test_setup(o[0], o[1], o[2], d[0], d[1], d[2], a, 200.0f);
                const rtx::LineTest Ts =
                    rtx::line_test_setup(o[0], rtx::kCullSy * o[1], o[2], d[0], dys, d[2], as, 200.0f * rtx::kCullSy);
                const rtx::LineTest Ws =
                    spec::line_test_setup(o[0], rtx::kCullSy * o[1], o[2], d[0], dys, d[2], as, 200.0f * rtx::kCullSy);
                const bool same = same_line(T, W) && same_line(Ts, Ws);
                if (!same && line_bad < 5)
                    fprintf(stderr, "line: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) ulp %d\n", o[0], o[1], o[2], d[0], d[1], d[2], u);
                line_bad += !same;
                if (u == 13) (W.thr == -INFINITY ? line_unsafe : line_safe) += 1;
            }
            rtx::pf_host_ulp[0] = rtx::pf_host_ulp[1] = rtx::pf_host_ulp[2] = 0;
            // the stretch and its items
            rtx::GridStretch S, Q;
            const bool s_ok = rtx::grid_stretch(L.G, o[0], o[1], o[2], d[0], d[1], d[2], S);
            const bool q_ok = spec::grid_stretch(L.G, o[0], o[1], o[2], d[0], d[1], d[2], Q);
            bool same = s_ok == q_ok && S.n == Q.n;
            if (same && q_ok && Q.n > 0u) same = same_stretch(S, Q);
            if (!same && st_bad < 5)
                fprintf(stderr, "stretch: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g): %d n %u, spec %d n %u\n", o[0], o[1], o[2],
                        d[0], d[1], d[2], (int)s_ok, S.n, (int)q_ok, Q.n);
            st_bad += !same;
            (!q_ok ? st_quit : Q.n == 0u ? st_none : st_items) += 1;
            mask_bad += rtx::grid_mask_items(L.G, cellf, o[0], o[1], o[2], d[0], d[1], d[2]) !=
                        spec::grid_mask_items(L.G, cellf, o[0], o[1], o[2], d[0], d[1], d[2]);
        }
    }
    const long failures = line_bad + st_bad + mask_bad;
    const bool fed = line_safe >= min_each && line_unsafe >= min_each && st_items >= min_each && st_none >= min_each &&
                     st_quit >= min_each && dy0_inside >= min_each && near_omax >= min_each;
    printf("{\"layers\": %ld, \"rays\": %ld, \"line_safe\": %ld, \"line_unsafe\": %ld, \"line_differ\": %ld, "
           "\"stretch_items\": %ld, \"stretch_none\": %ld, \"stretch_gave_up\": %ld, \"stretch_differ\": %ld, "
           "\"mask_differ\": %ld, \"dy0_inside_slab\": %ld, \"near_omax\": %ld, \"min_each\": %ld, \"failures\": %ld}\n",
           layers, rays, line_safe, line_unsafe, line_bad, st_items, st_none, st_quit, st_bad, mask_bad, dy0_inside,
           near_omax, min_each, failures);
    return failures == 0 && fed ? 0 : 1;
}
