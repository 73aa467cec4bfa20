// grid_coop_check.cpp — CPU check of the wave-cooperative walk of the layer
// grid (raytrace-we-gpu_amd/csrc/rtx_grid.h: grid_stretch, grid_item_cells,
// grid_share_mark), with the header's own code.
//
// 1. Superset. For the layers and adversarial rays of grid_check.cpp (the
//    RTIOW layer and random ones; rays near-tangent to a sphere at every slope
//    down to grazing the layer, aimed at cell corners and edges, along the
//    axes or level (a d component exactly 0), leaving a sphere's surface,
//    origins on the slab's and the box's faces) plus random rays: wherever the
//    DDA (grid_walk) applies and the items do not give up, every cell the DDA
//    visits is a cell of some item. At least min_checked such rays, no miss.
//    Built with -DRTX_GRID_COOP_EPS=0 the same run must miss (the test's
//    sensitivity leg).
// 2. Bloat: the summed popcount of the items' block masks over the DDA's.
// 3. The wave's sharing: a host emulation of the 64-lane distribution (the
//    prefix sum over the active lanes, the owners' marks, the rounds) must
//    reproduce the OR of the per-ray masks — for waves without items, one
//    lane holding every item over several rounds, totals of 63, 64, 65 and
//    128, inactive lanes in between, a give-up lane among normal ones (~0),
//    and random waves.
// 4. Hostile mode (argv[4] = k > 0): a quarter of every layer's spheres are
//    made degenerate and every k-th ray becomes the next hostile class of
//    tests/hostile_rays.h (NaN, infinite, zero, tiny and huge components). A
//    ray inside the line test's safe range is checked like any other; one
//    outside it, which the kernel never walks, still goes through grid_walk,
//    grid_stretch and grid_item_cells: every cell index must lie inside the
//    grid (hostile_cells_outside), and a wave with such a lane gives up.
// Prints one JSON line; exit status 1 on a miss, on too few rays, on a wave
// whose emulation differs, or on a cell index outside the grid.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma grid_coop_check.cpp
#include <bitset>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_grid.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_prefilter.h"
#include "hostile_rays.h"

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

static bool make_layer(Layer &L, bool rtiow, bool degenerate) {
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
    if (degenerate)
        for (uint32_t j = 1; j < (uint32_t)(L.s.size() / 4); ++j)
            if (uni() < 0.25) hostile::degenerate_sphere(L.s.data(), j, (int)(uni() * 6.0), true);
    return rtx::build_layer_grid(L.s.data(), 0u, (uint32_t)(L.s.size() / 4), L.G, L.cell);
}

// One adversarial or random ray of the layer; false when the draw is dropped.
static bool make_ray(const Layer &L, Ray &R) {
    const uint32_t n = (uint32_t)(L.s.size() / 4);
    const float *c = &L.s[4 * (size_t)(uni() * n)];
    const float y0 = L.s[1];
    const double r = c[3];
    double dir[3], o[3];
    const int kind = (int)(uni() * 7.0);
    unit(dir);
    if (uni() < 0.4) dir[1] = std::pow(10.0, -7.0 + 6.0 * uni()) * sym();  // grazing the layer
    if (kind == 3) {  // along an axis or level
        const int z = (int)(uni() * 3.0);
        dir[z == 0 ? 0 : z == 1 ? 2 : 1] = 0.0;
        if (uni() < 0.3) dir[z == 0 ? 2 : 0] = 0.0;  // two components 0
    }
    const double xlo = L.G.x0, xhi = L.G.x0 + (double)L.G.nx * L.G.h, zlo = L.G.z0, zhi = L.G.z0 + (double)L.G.nz * L.G.h;
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
    if (on > 63.9) return false;
    const double dn = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    if (!(dn > 0.0)) return false;
    const double dlen = std::pow(10.0, -2.0 + 4.0 * uni()) / dn;
    for (int i = 0; i < 3; ++i) R.o[i] = (float)o[i], R.d[i] = (float)(dir[i] * dlen);
    return true;
}

typedef std::bitset<rtx::kGridMaxCells> CellSet;

// the cells of the ray's items; false: the lane gives up
static bool item_cells(const rtx::LayerGrid &G, const Ray &r, CellSet &cs, uint32_t *items = nullptr) {
    rtx::GridStretch S;
    if (!rtx::grid_stretch(G, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], S)) return false;
    if (items) *items = S.n;
    for (uint32_t i = 0; i < S.n; ++i) {
        uint32_t k0, stride, cnt;
        rtx::grid_item_cells(G, S.lo, S.hi, S.A, S.s, S.zmajor, S.c0 + i, k0, stride, cnt);
        for (uint32_t q = 0; q < cnt; ++q) cs.set(k0 + q * stride);
    }
    return true;
}

// The wave as the kernel runs it (rtx_kernels.hip grid_wave_mask): `act` the
// lanes that take part, `bad` lanes outside the line test's safe range.
// *fault is set when a slot finds no owner or a wrong one.
static uint64_t wave_emulate(const Layer &L, const Ray *rays, uint64_t act, uint64_t bad, uint32_t *rounds_out,
                             bool *fault) {
    rtx::GridStretch S[64];
    bool giveup = false;
    for (int l = 0; l < 64; ++l) {
        if (!((act >> l) & 1ull)) continue;
        const Ray &r = rays[l];
        if (((bad >> l) & 1ull) || !rtx::grid_stretch(L.G, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], S[l]))
            giveup = true;
    }
    *rounds_out = 0;
    if (giveup) return ~0ull;
    uint32_t nact = 0, slot[64], start[64], total = 0;
    for (int l = 0; l < 64; ++l) {
        if (!((act >> l) & 1ull)) continue;
        slot[l] = nact++;
        start[l] = total;
        total += S[l].n;
    }
    uint64_t mine[64] = {0};
    for (uint32_t base = 0; base < total; base += nact) {
        ++*rounds_out;
        uint32_t marks[64] = {0};
        for (int l = 0; l < 64; ++l) {
            if (!((act >> l) & 1ull)) continue;
            const int ms = rtx::grid_share_mark(start[l], S[l].n, base, nact);
            if (ms >= 0) {
                if (marks[ms] != 0u) *fault = true;  // two owners at one slot
                marks[ms] = (uint32_t)l + 1u;
            }
        }
        for (int l = 0; l < 64; ++l) {
            if (!((act >> l) & 1ull) || !(base + slot[l] < total)) continue;
            int at = (int)slot[l];
            while (at >= 0 && marks[at] == 0u) --at;
            if (at < 0) {
                *fault = true;
                continue;
            }
            const uint32_t own = marks[at] - 1u, item = base + slot[l];
            if (!(item >= start[own] && item < start[own] + S[own].n)) {
                *fault = true;
                continue;
            }
            uint32_t k0, stride, cnt;
            rtx::grid_item_cells(L.G, S[own].lo, S[own].hi, S[own].A, S[own].s, S[own].zmajor,
                                 S[own].c0 + (item - start[own]), k0, stride, cnt);
            for (uint32_t q = 0; q < cnt; ++q) mine[l] |= L.cell[k0 + q * stride];
        }
    }
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= mine[l];
    return m;
}

int main(int argc, char **argv) {
    const long nlayers = argc > 1 ? atol(argv[1]) : 400;
    const long nrays = argc > 2 ? atol(argv[2]) : 4000;
    const long min_checked = argc > 3 ? atol(argv[3]) : 1000000;
    const long hostile_every = argc > 4 ? atol(argv[4]) : 0;
    long hostile_rays = 0, hostile_walked = 0, hostile_gave_up = 0, hostile_outside = 0;
    int hostile_cls = 0;
    long rays = 0, checked = 0, dda_all = 0, item_all = 0, missed_rays = 0, missed_cells = 0, layers = 0;
    double dda_bits = 0.0, item_bits = 0.0, dda_cells = 0.0, item_cells_n = 0.0, items_n = 0.0;
    long waves = 0, wave_bad = 0, wave_rounds = 0;
    for (long li = 0; li < nlayers; ++li) {
        Layer L;
        if (!make_layer(L, li % 3 == 0, hostile_every > 0)) continue;
        ++layers;
        auto cellf = [&L](uint32_t k) { return (uint64_t)L.cell[k]; };
        // rays by item count, for the waves below
        std::vector<Ray> by_n[4], none, quit, longest, hostile_quit;
        uint32_t longest_n = 0;
        for (long k = 0; k < nrays; ++k) {
            Ray r;
            if (!make_ray(L, r)) continue;
            ++rays;
            const bool hz = hostile_every > 0 && k % hostile_every == 0;
            if (hz) {
                hostile::hostile_ray(hostile_cls++, &L.s[4 * (size_t)(uni() * (double)(L.s.size() / 4))], r.o, r.d);
                ++hostile_rays;
            }
            const float a = fmaf(r.d[2], r.d[2], fmaf(r.d[1], r.d[1], r.d[0] * r.d[0]));
            const rtx::LineTest T = rtx::line_test_setup(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], a, 200.0f);
            if (T.thr == -INFINITY) {
                if (hz) {  // never walked by the kernel: both walks must still end, inside the grid
                    ++hostile_walked;
                    const uint32_t ncell = L.G.nx * L.G.nz;
                    const bool w_ok = rtx::grid_walk(L.G, rtx::kGridMaxSteps, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1],
                                                     r.d[2], INFINITY, [&](uint32_t c) {
                                                         hostile_outside += c >= ncell;
                                                         return true;
                                                     });
                    rtx::GridStretch S;
                    const bool s_ok = rtx::grid_stretch(L.G, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], S);
                    if (s_ok) {
                        if (S.n > rtx::kGridMaxSteps) ++hostile_outside;
                        for (uint32_t i = 0; i < S.n && i < rtx::kGridMaxSteps; ++i) {
                            uint32_t k0, stride, cnt;
                            rtx::grid_item_cells(L.G, S.lo, S.hi, S.A, S.s, S.zmajor, S.c0 + i, k0, stride, cnt);
                            for (uint32_t q = 0; q < cnt; ++q) hostile_outside += k0 + q * stride >= ncell;
                        }
                    } else if (hostile_quit.size() < 4) {
                        hostile_quit.push_back(r);
                    }
                    hostile_gave_up += !w_ok + !s_ok;
                }
                continue;
            }
            CellSet dda, itm;
            const bool dda_ok = rtx::grid_walk(L.G, rtx::kGridMaxSteps, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2],
                                               INFINITY, [&](uint32_t c) { return dda.set(c), true; });
            uint32_t ni = 0;
            const bool itm_ok = item_cells(L.G, r, itm, &ni);
            if (!itm_ok && quit.size() < 4) quit.push_back(r);
            if (itm_ok && ni == 0 && none.size() < 64) none.push_back(r);
            if (itm_ok && ni >= 1 && ni <= 3 && by_n[ni].size() < 64) by_n[ni].push_back(r);
            if (itm_ok && ni > longest_n) longest_n = ni, longest.assign(1, r);
            if (!dda_ok) {
                ++dda_all;
                continue;
            }
            if (!itm_ok) {
                ++item_all;  // every block: contains the DDA's trivially, not counted as checked
                continue;
            }
            ++checked;
            const CellSet miss = dda & ~itm;
            if (miss.any()) {
                if (missed_rays < 5)
                    fprintf(stderr, "miss: %zu cells, o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) h %g\n", miss.count(),
                            r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], L.G.h);
                ++missed_rays;
                missed_cells += (long)miss.count();
            }
            dda_cells += (double)dda.count(), item_cells_n += (double)itm.count(), items_n += ni;
            dda_bits += (double)__builtin_popcountll(rtx::grid_mask(L.G, cellf, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2]));
            const uint64_t mi = rtx::grid_mask_items(L.G, cellf, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2]);
            uint64_t want = 0;
            for (uint32_t c = 0; c < L.G.nx * L.G.nz; ++c)
                if (itm.test(c)) want |= L.cell[c];
            if (mi != want) ++wave_bad;  // grid_mask_items is the items' cells
            item_bits += (double)__builtin_popcountll(mi);
        }
        // the wave's sharing
        auto run_wave = [&](const Ray *w, uint64_t act, uint64_t bad, int want_total, bool want_all) {
            uint64_t want = 0;
            uint32_t total = 0;
            for (int l = 0; l < 64; ++l) {
                if (!((act >> l) & 1ull)) continue;
                rtx::GridStretch S;
                const bool ok = !((bad >> l) & 1ull) &&
                                rtx::grid_stretch(L.G, w[l].o[0], w[l].o[1], w[l].o[2], w[l].d[0], w[l].d[1], w[l].d[2], S);
                want |= ok ? rtx::grid_mask_items(L.G, cellf, w[l].o[0], w[l].o[1], w[l].o[2], w[l].d[0], w[l].d[1], w[l].d[2])
                           : ~0ull;
                total += ok ? S.n : 0u;
            }
            uint32_t rounds = 0;
            bool fault = false;
            const uint64_t got = wave_emulate(L, w, act, bad, &rounds, &fault);
            const uint32_t nact = (uint32_t)__builtin_popcountll(act);
            ++waves;
            wave_rounds += rounds;
            bool ok = got == want && !fault;
            if (want_all) ok = ok && got == ~0ull;
            if (!want_all && want != ~0ull) ok = ok && rounds == (nact ? (total + nact - 1) / nact : 0u);
            if (want_total >= 0) ok = ok && (int)total == want_total;
            if (!ok) {
                if (wave_bad < 5) fprintf(stderr, "wave: got %llx want %llx total %u rounds %u fault %d\n",
                                          (unsigned long long)got, (unsigned long long)want, total, rounds, (int)fault);
                ++wave_bad;
            }
        };
        Ray w[64];
        const bool have = none.size() >= 1 && by_n[1].size() >= 1 && by_n[2].size() >= 1 && !longest.empty();
        if (have) {
            auto pick = [](const std::vector<Ray> &v, int l) { return v[(size_t)l % v.size()]; };
            for (int l = 0; l < 64; ++l) w[l] = pick(none, l);
            run_wave(w, ~0ull, 0ull, 0, false);  // no lane has an item
            run_wave(w, 0ull, 0ull, 0, false);   // (no lane at all)
            // one lane holds every item; 1, 4 and 64 lanes take part: its owner spans several rounds
            for (int l = 0; l < 64; ++l) w[l] = pick(none, l);
            w[37] = longest[0];
            run_wave(w, 1ull << 37, 0ull, (int)longest_n, false);
            run_wave(w, (1ull << 3) | (1ull << 20) | (1ull << 37) | (1ull << 63), 0ull, (int)longest_n, false);
            run_wave(w, ~0ull, 0ull, (int)longest_n, false);
            // totals of 63, 64, 65 and 128 over a full wave
            for (int l = 0; l < 64; ++l) w[l] = pick(by_n[1], l);
            run_wave(w, ~0ull, 0ull, 64, false);
            run_wave(w, ~0ull >> 1, 0ull, 63, false);  // lane 63 inactive
            w[63] = pick(none, 0);
            run_wave(w, ~0ull, 0ull, 63, false);
            w[63] = pick(by_n[2], 0);
            run_wave(w, ~0ull, 0ull, 65, false);
            for (int l = 0; l < 64; ++l) w[l] = pick(by_n[2], l);
            run_wave(w, ~0ull, 0ull, 128, false);
            // inactive lanes in between: every other lane, a single live lane, 128 items over 32 lanes
            run_wave(w, 0x5555555555555555ull, 0ull, 64, false);
            run_wave(w, 1ull, 0ull, 2, false);
            for (int l = 0; l < 64; ++l) w[l] = l % 2 ? pick(by_n[1], l) : pick(by_n[3].empty() ? by_n[1] : by_n[3], l);
            run_wave(w, 0xf0f0f0f00f0f0f0full, 0ull, -1, false);
            // a give-up lane among normal ones: outside the line test's range, or a ray the items give up on
            run_wave(w, ~0ull, 1ull << 17, -1, true);
            if (!quit.empty()) {
                w[5] = quit[0];
                run_wave(w, ~0ull, 0ull, -1, true);
            }
            for (size_t q = 0; q < hostile_quit.size(); ++q) {  // a hostile lane among normal ones
                w[9 + q] = hostile_quit[q];
                run_wave(w, ~0ull, 0ull, -1, true);
            }
            // random waves
            for (int rep = 0; rep < 40; ++rep) {
                for (int l = 0; l < 64; ++l) {
                    const double u = uni();
                    w[l] = u < 0.4 ? pick(none, (int)(uni() * 64)) : u < 0.7 ? pick(by_n[1], (int)(uni() * 64))
                           : u < 0.9 ? pick(by_n[2], (int)(uni() * 64)) : longest[0];
                }
                uint64_t act = g_s;
                uni();
                if (rep % 4 == 0) act = ~0ull;
                if (rep % 4 == 1) act &= g_s, uni();
                run_wave(w, act, 0ull, -1, false);
            }
        }
    }
    const bool ok = missed_rays == 0 && checked >= min_checked && wave_bad == 0 && waves > 0 && hostile_outside == 0;
    printf("{\"layers\": %ld, \"rays\": %ld, \"checked\": %ld, \"min_checked\": %ld, \"dda_every_block\": %ld, "
           "\"items_every_block\": %ld, \"missed_rays\": %ld, \"missed_cells\": %ld, \"cells_dda\": %.3f, "
           "\"cells_items\": %.3f, \"items_per_ray\": %.3f, \"block_mask_bloat\": %.5f, \"waves\": %ld, "
           "\"wave_rounds\": %ld, \"waves_wrong\": %ld, \"eps\": %g, \"hostile_rays\": %ld, \"hostile_walked\": %ld, "
           "\"hostile_gave_up\": %ld, \"hostile_cells_outside\": %ld, \"failures\": %ld}\n",
           layers, rays, checked, min_checked, dda_all, item_all, missed_rays, missed_cells,
           checked ? dda_cells / (double)checked : 0.0, checked ? item_cells_n / (double)checked : 0.0,
           checked ? items_n / (double)checked : 0.0, dda_bits > 0.0 ? item_bits / dda_bits : 0.0, waves, wave_rounds,
           wave_bad, (double)rtx::kGridCoopEps, hostile_rays, hostile_walked, hostile_gave_up, hostile_outside,
           missed_rays + wave_bad + hostile_outside);
    return ok ? 0 : 1;
}
