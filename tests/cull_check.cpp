// cull_check.cpp — CPU check of the culled layout of large scenes
// (raytrace-we-gpu_amd/csrc/rtx_cull.h) on the layouts
// build_cull really makes, with the header's own code: Morton order, padding
// copies with R = -inf, the flat section aligned to 512 blocks, three levels
// of bounds. tests/test_cull_cases.py feeds it the worlds and cameras of
// tests/cull_cases.py.
//
// Input (argv[1]), little endian: uint32 n, uint32 nrays, uint32 nprim,
// uint32 0; n * 4 floats (cx, cy, cz, r); nrays * 6 floats (origin,
// direction). The scene-order `pre` records, smag and the scene-order flat
// run are made as rtx_upload_world makes them. With argv[2], the layout's
// position map is written there (uint32 perm[positions], uint8 pad[positions]).
//
// 1. Layout invariants: every scene index at exactly one non-padding
//    position; a padding position copies its section's last sphere and has
//    R = -inf; a real position's record is the sphere's `pre` record; a bound
//    has R = -inf iff all its positions are padding; flat_lo is 0, nblk or a
//    multiple of 512; every position from flat_lo on has the flat height's
//    bits and none before it has, except large spheres (section 0).
// 2. Conservativeness, at all three bound sizes: for every ray, t_min 1e-3 and
//    1e-6, and every sphere the reference's fp32 test accepts (disc >= 0 and a
//    root in [t_min, inf), as prefilter_check.cpp computes it), the sphere's
//    own prefilter test must flag it and its block (8), group (64) and
//    super-group (512) bounds must each pass the line test and the half test —
//    with the ops the kernels run (rtx_kernels.hip scan_culled: the 5-op test
//    of the stretched ray for flat bounds, the 7-op one otherwise;
//    hit_world_groups_culled: the 7-op order everywhere), the line basis's
//    hardware rsq/sqrt exact or one ulp off either way. A miss is a failure.
// 3. The walk of scan_culled for one lane (no wave OR), over the first nprim
//    rays at t_min 1e-3: bounds passed and failed at each level, flat and not
//    (padding bounds, R = -inf, counted apart: they fail for every ray inside
//    the prefilter's safe range), bounds the half test alone rejects, blocks
//    stepped, blocks with a flagged sphere (list entries), and the rays with
//    more than 24 of either.
// Prints one JSON line; exit status 1 on a malformed input or a failed check.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma cull_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_cull.h"

// hit_world32's acceptance of one sphere (oracle/rtx_oracle.c), reference op order, best = +inf
static bool ref_accepts(const float o[3], const float d[3], const float *c, float negr2, float a, float t_min) {
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

// A ray's per-segment values, as hit_world_culled and hit_world_groups_culled set them up.
struct RaySetup {
    rtx::LineTest T, Ts;
    rtx::HalfTest H, Hs;
    rtx::LineFlat K, Ks;
    float thr_b, thr_bs, kws;
};
static RaySetup setup(const float *q, float a, float smag, float flat_cy, float t_min) {
    RaySetup R;
    R.T = rtx::line_test_setup(q[0], q[1], q[2], q[3], q[4], q[5], a, smag);
    // line_test_stretched, half_test_stretched (rtx_kernels.hip)
    const float dys = rtx::kCullSy * q[4];
    const float as = fmaf(q[5], q[5], fmaf(dys, dys, q[3] * q[3]));
    R.Ts = rtx::line_test_setup(q[0], rtx::kCullSy * q[1], q[2], q[3], dys, q[5], as, smag * rtx::kCullSy);
    R.thr_b = R.T.thr * rtx::kCullThrScale;
    R.thr_bs = R.Ts.thr * rtx::kCullThrScaleSy;
    R.H = rtx::half_test_setup(q[0], q[1], q[2], q[3], q[4], q[5], a, R.thr_b, t_min);
    R.Hs = rtx::half_test_setup(q[0], rtx::kCullSy * q[1], q[2], q[3], dys, q[5], as, R.thr_bs, t_min);
    R.K = rtx::line_test_flat(R.T, flat_cy);
    R.Ks = rtx::line_test_flat(R.Ts, rtx::kCullSy * flat_cy);
    R.kws = rtx::half_test_kw(R.Hs, rtx::kCullSy * flat_cy);
    return R;
}
// Entry e of a level's AoSoA-8 array.
static const float *entry(const std::vector<float> &arr, uint32_t e) { return &arr[32 * (size_t)(e >> 3) + (e & 7u)]; }
// scan_culled's test of one bound: bit 0 the line test, bit 1 the half test.
static int lane_bound(const RaySetup &R, const float *b, bool flat) {
    if (flat) {
        const float q = rtx::line_test_q_flat(R.Ts, R.Ks, b[0], b[16], b[24]);
        const float pw = rtx::half_test_pw_flat(R.Hs, R.kws, b[0], b[16]);
        return (!(q < R.thr_bs) ? 1 : 0) | (rtx::half_test_pass(pw, rtx::half_test_q2(R.Hs, pw, b[24])) ? 2 : 0);
    }
    const float q = rtx::line_test_q(R.T, b[0], b[8], b[16], b[24]);
    const float pw = rtx::half_test_pw(R.H, b[0], b[8], b[16]);
    return (!(q < R.thr_b) ? 1 : 0) | (rtx::half_test_pass(pw, rtx::half_test_q2(R.H, pw, b[24])) ? 2 : 0);
}
// hit_world_groups_culled's (bound_pass, block_mask: the 7-op order, stretched for flat bounds)
static int coop_bound(const RaySetup &R, const float *b, bool flat) {
    const rtx::LineTest &L = flat ? R.Ts : R.T;
    const rtx::HalfTest &Hh = flat ? R.Hs : R.H;
    const float q = rtx::line_test_q(L, b[0], b[8], b[16], b[24]);
    const float pw = rtx::half_test_pw(Hh, b[0], b[8], b[16]);
    return (!(q < (flat ? R.thr_bs : R.thr_b)) ? 1 : 0) | (rtx::half_test_pass(pw, rtx::half_test_q2(Hh, pw, b[24])) ? 2 : 0);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: cull_check CASE.bin\n");
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    uint32_t head[4] = {0, 0, 0, 0};
    if (fread(head, sizeof(uint32_t), 4, f) != 4 || head[0] == 0 || head[0] > (1u << 20) || head[1] > (1u << 24) ||
        head[2] > head[1]) {
        fprintf(stderr, "cull_check: bad header\n");
        return 1;
    }
    const uint32_t n = head[0], nrays = head[1], nprim = head[2];
    std::vector<float> sph(4 * (size_t)n), rays(6 * (size_t)nrays);
    if (fread(sph.data(), sizeof(float), sph.size(), f) != sph.size() ||
        fread(rays.data(), sizeof(float), rays.size(), f) != rays.size()) {
        fprintf(stderr, "cull_check: short file\n");
        return 1;
    }
    fclose(f);

    // rtx_upload_world: the scene-order records, smag, the longest run of flat blocks
    std::vector<float> pre4(4 * (size_t)n);
    double smag_d = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float *s = &sph[4 * (size_t)i];
        const float r2 = s[3] * s[3];
        pre4[4 * i] = s[0], pre4[4 * i + 1] = s[1], pre4[4 * i + 2] = s[2];
        pre4[4 * i + 3] = rtx::prefilter_R(s[0], s[1], s[2], r2);
        smag_d = std::max(smag_d, std::sqrt((double)s[0] * s[0] + (double)s[1] * s[1] + (double)s[2] * s[2]) +
                                      std::fabs((double)s[3]));
    }
    float smag = (float)smag_d;
    if ((double)smag < smag_d) smag = std::nextafter(smag, INFINITY);
    uint32_t run_lo = 0, run_hi = 0;
    float flat_cy = 0.0f;
    {
        const uint32_t nb = (n + 7) / 8;
        auto bits = [&](uint32_t b, int k) { return rtx::cull_bits(sph[4 * (size_t)std::min(8 * b + (uint32_t)k, n - 1) + 1]); };
        auto flat = [&](uint32_t b) {
            for (int k = 1; k < 8; ++k)
                if (bits(b, k) != bits(b, 0)) return false;
            return true;
        };
        for (uint32_t b = 0; b < nb;) {
            if (!flat(b)) {
                ++b;
                continue;
            }
            uint32_t e = b + 1;
            while (e < nb && flat(e) && bits(e, 0) == bits(b, 0)) ++e;
            if (e - b > run_hi - run_lo) run_lo = b, run_hi = e, flat_cy = sph[4 * (size_t)std::min(8 * b, n - 1) + 1];
            b = e;
        }
    }
    const bool has_flat = run_hi > run_lo;
    const rtx::CullLayout L = rtx::build_cull(sph.data(), n, pre4.data(), has_flat, flat_cy);
    const uint32_t np = (uint32_t)L.perm.size(), nblk = np / 8, ngrp = (nblk + 7) / 8, nsg = (ngrp + 7) / 8,
                   nhg = (nsg + 7) / 8;
    const uint32_t flat_lo = L.flat_lo;
    if (argc > 2) {  // the position map, for the caller: uint32 perm[np], uint8 pad[np]
        FILE *g = fopen(argv[2], "wb");
        if (!g || fwrite(L.perm.data(), sizeof(uint32_t), np, g) != np || fwrite(L.pad.data(), 1, np, g) != np) {
            perror(argv[2]);
            return 1;
        }
        fclose(g);
    }

    // ---- 1. layout invariants ----
    long bad_size = 0, bad_perm = 0, bad_pad = 0, bad_record = 0, bad_bound = 0, bad_flat_lo = 0, bad_height = 0;
    if (np % 8 != 0 || L.pad.size() != np || L.pre.size() != 4 * (size_t)np || L.bnd.size() != 32 * (size_t)ngrp ||
        L.bnd2.size() != 32 * (size_t)nsg || L.bnd3.size() != 32 * (size_t)nhg)
        ++bad_size;
    std::vector<float> rs(n);
    for (uint32_t i = 0; i < n; ++i) rs[i] = std::fabs(sph[4 * (size_t)i + 3]);
    std::sort(rs.begin(), rs.end());
    const float big = 8.0f * rs[n / 2];
    std::vector<uint32_t> seen(n, 0), pos_of(n, 0);
    uint32_t sec_count[3] = {0, 0, 0};
    uint32_t last_real = ~0u;
    for (uint32_t p = 0; p < np && !bad_size; ++p) {
        const uint32_t i = L.perm[p];
        if (i >= n) {
            ++bad_perm;
            continue;
        }
        const float *rec = &L.pre[32 * (size_t)(p / 8)];
        const float R = rec[24 + p % 8];
        const bool large = std::fabs(sph[4 * (size_t)i + 3]) > big;
        const bool layer = has_flat && rtx::cull_bits(sph[4 * (size_t)i + 1]) == rtx::cull_bits(flat_cy);
        if (L.pad[p]) {
            // a copy of the last real sphere before it (its section's last), never flagged
            if (last_real == ~0u || i != L.perm[last_real] || !(R == -INFINITY)) ++bad_pad;
        } else {
            if (seen[i]++ == 0) pos_of[i] = p;
            last_real = p;
            ++sec_count[large ? 0 : layer ? 2 : 1];
            if (rtx::cull_bits(R) != rtx::cull_bits(pre4[4 * (size_t)i + 3])) ++bad_record;
        }
        for (int k = 0; k < 3; ++k)
            if (rtx::cull_bits(rec[8 * k + p % 8]) != rtx::cull_bits(sph[4 * (size_t)i + k])) ++bad_record;
        if (p / 8 >= flat_lo ? (!layer || large) : (layer && !large)) ++bad_height;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (seen[i] != 1) ++bad_perm;
    if (!(flat_lo == 0 || flat_lo == nblk || flat_lo % rtx::kCullAlign == 0) || flat_lo > nblk) ++bad_flat_lo;
    // a bound of positions [p0, p1) has R = -inf iff they are all padding
    auto all_pad = [&](uint32_t p0, uint32_t p1) {
        for (uint32_t p = p0; p < std::min(p1, np); ++p)
            if (!L.pad[p]) return false;
        return true;
    };
    if (!bad_size) {
        for (uint32_t b = 0; b < nblk; ++b)
            if ((entry(L.bnd, b)[24] == -INFINITY) != all_pad(8 * b, 8 * b + 8) || !(entry(L.bnd, b)[24] < INFINITY))
                ++bad_bound;
        for (uint32_t g = 0; g < ngrp; ++g)
            if ((entry(L.bnd2, g)[24] == -INFINITY) != all_pad(64 * g, 64 * g + 64) || !(entry(L.bnd2, g)[24] < INFINITY))
                ++bad_bound;
        for (uint32_t s = 0; s < nsg; ++s)
            if ((entry(L.bnd3, s)[24] == -INFINITY) != all_pad(512 * s, 512 * s + 512) ||
                !(entry(L.bnd3, s)[24] < INFINITY))
                ++bad_bound;
    }
    const long layout_failures = bad_size + bad_perm + bad_pad + bad_record + bad_bound + bad_flat_lo + bad_height;

    // ---- 2. conservativeness on this layout ----
    long accepted = 0, sphere_missed = 0, miss[3] = {0, 0, 0}, unsafe = 0;
    const std::vector<float> *level[3] = {&L.bnd, &L.bnd2, &L.bnd3};
    const float t_mins[2] = {1e-3f, 1e-6f};
    for (uint32_t r = 0; r < nrays && !layout_failures; ++r) {
        const float *q = &rays[6 * (size_t)r];
        const float a = fmaf(q[5], q[5], fmaf(q[4], q[4], q[3] * q[3]));
        for (int ti = 0; ti < 2; ++ti) {
            RaySetup R[3];
            bool made = false;
            for (uint32_t i = 0; i < n; ++i) {
                const float *c = &sph[4 * (size_t)i];
                if (!ref_accepts(q, q + 3, c, -(c[3] * c[3]), a, t_mins[ti])) continue;
                ++accepted;
                if (!made) {
                    for (int u = 0; u < 3; ++u) {
                        rtx::pf_host_ulp[0] = rtx::pf_host_ulp[1] = rtx::pf_host_ulp[2] = u - 1;
                        R[u] = setup(q, a, smag, flat_cy, t_mins[ti]);
                    }
                    made = true;
                    unsafe += R[1].T.thr == -INFINITY;
                }
                const uint32_t p = pos_of[i], b = p / 8;
                const float *rec = &L.pre[32 * (size_t)b + p % 8];
                bool s_ok = true, l_ok[3] = {true, true, true};
                for (int u = 0; u < 3; ++u) {
                    // the sphere: scan_culled's step (5 ops on a flat block), the coop's 7 ops
                    const float q7 = rtx::line_test_q(R[u].T, rec[0], rec[8], rec[16], rec[24]);
                    const float ql = b >= flat_lo ? rtx::line_test_q_flat(R[u].T, R[u].K, rec[0], rec[16], rec[24]) : q7;
                    s_ok = s_ok && !(q7 < R[u].T.thr) && !(ql < R[u].T.thr);
                    // its bounds: entry p >> (3, 6, 9), flat by the first block of the row of 8 (scan_culled's
                    // bound_mask, the coop's bounds_mask) or of the entry (the coop's test_entry): the same
                    // thing while flat_lo is aligned, which the invariants above have checked
                    for (int lv = 0; lv < 3; ++lv) {
                        const uint32_t e = p >> (3 * lv + 3);
                        const bool flat = ((e & ~7u) << (3 * lv)) >= flat_lo;
                        const bool flat_e = (e << (3 * lv)) >= flat_lo;
                        const float *bd = entry(*level[lv], e);
                        l_ok[lv] = l_ok[lv] && lane_bound(R[u], bd, flat) == 3 && coop_bound(R[u], bd, flat_e) == 3;
                    }
                }
                if (!s_ok && ++sphere_missed <= 5)
                    fprintf(stderr, "SPHERE MISS sphere %u position %u ray %u t_min %g\n", i, p, r, (double)t_mins[ti]);
                for (int lv = 0; lv < 3; ++lv)
                    if (!l_ok[lv] && ++miss[lv] <= 5)
                        fprintf(stderr, "BOUND MISS level %d sphere %u position %u ray %u t_min %g\n", lv + 1, i, p, r,
                                (double)t_mins[ti]);
            }
        }
    }
    rtx::pf_host_ulp[0] = rtx::pf_host_ulp[1] = rtx::pf_host_ulp[2] = 0;

    // ---- 3. scan_culled's walk, one lane ----
    // [level 1..3][flat][0 failed, 1 passed]; padding bounds (R = -inf) apart
    long walk[3][2][2] = {}, pad_failed[3] = {0, 0, 0}, pad_passed = 0, half_only = 0, blocks_stepped = 0, entries = 0;
    long rays_over_24_blocks = 0, rays_over_24_entries = 0;
    auto first_bits = [](uint32_t k) { return k >= 8u ? 0xffu : (1u << k) - 1u; };
    for (uint32_t r = 0; r < nprim && !layout_failures; ++r) {
        const float *q = &rays[6 * (size_t)r];
        const float a = fmaf(q[5], q[5], fmaf(q[4], q[4], q[3] * q[3]));
        const RaySetup R = setup(q, a, smag, flat_cy, 1e-3f);
        // the 8 bounds of a row whose entries cover blocks from b0 on
        auto bound_mask = [&](const std::vector<float> &arr, uint32_t row, uint32_t b0, uint32_t live, int lv) {
            const bool flat = b0 >= flat_lo;
            uint32_t m = 0;
            for (uint32_t j = 0; j < 8; ++j) {
                if (!((live >> j) & 1u)) continue;
                const float *bd = &arr[32 * (size_t)row + j];
                const int t = lane_bound(R, bd, flat);
                if (t == 3) m |= 1u << j;
                if (bd[24] == -INFINITY) {  // passes only for a ray outside the prefilter's safe range
                    if (t == 3)
                        ++pad_passed;
                    else
                        ++pad_failed[lv];
                    continue;
                }
                ++walk[lv][flat][t == 3];
                half_only += t == 1;
            }
            return m;
        };
        long stepped = 0, ent = 0;
        for (uint32_t hg = 0; hg < nhg; ++hg) {
            uint32_t m3 = bound_mask(L.bnd3, hg, 512u * hg, first_bits(nsg - 8u * hg), 2);
            for (; m3; m3 &= m3 - 1u) {
                const uint32_t sg = 8u * hg + (uint32_t)__builtin_ctz(m3);
                uint32_t m2 = bound_mask(L.bnd2, sg, 64u * sg, first_bits(ngrp - 8u * sg), 1);
                for (; m2; m2 &= m2 - 1u) {
                    const uint32_t g = 8u * sg + (uint32_t)__builtin_ctz(m2);
                    uint32_t m1 = bound_mask(L.bnd, g, 8u * g, first_bits(nblk - 8u * g), 0);
                    for (; m1; m1 &= m1 - 1u) {
                        const uint32_t bb = 8u * g + (uint32_t)__builtin_ctz(m1);
                        ++stepped;
                        const float *blk = &L.pre[32 * (size_t)bb];
                        bool any = false;
                        for (int j = 0; j < 8; ++j) {
                            const float qq = bb >= flat_lo
                                                 ? rtx::line_test_q_flat(R.T, R.K, blk[j], blk[16 + j], blk[24 + j])
                                                 : rtx::line_test_q(R.T, blk[j], blk[8 + j], blk[16 + j], blk[24 + j]);
                            any = any || !(qq < R.T.thr);
                        }
                        ent += any;
                    }
                }
            }
        }
        blocks_stepped += stepped;
        entries += ent;
        rays_over_24_blocks += stepped > 24;
        rays_over_24_entries += ent > 24;
    }

    const long failures = layout_failures + sphere_missed + miss[0] + miss[1] + miss[2];
    printf("{\"n\": %u, \"rays\": %u, \"primary\": %u, \"has_flat\": %d, \"flat_cy\": %.9g, \"positions\": %u, "
           "\"flat_lo\": %u, \"nblk\": %u, \"ngrp\": %u, \"nsg\": %u, \"nhg\": %u, \"large\": %u, \"other\": %u, "
           "\"flat\": %u, \"bad_size\": %ld, \"bad_perm\": %ld, \"bad_pad\": %ld, \"bad_record\": %ld, "
           "\"bad_bound\": %ld, \"bad_flat_lo\": %ld, \"bad_height\": %ld, \"accepted\": %ld, \"unsafe_rays\": %ld, "
           "\"sphere_missed\": %ld, \"block_missed\": %ld, \"group_missed\": %ld, \"super_missed\": %ld, ",
           n, nrays, nprim, has_flat ? 1 : 0, (double)flat_cy, np, flat_lo, nblk, ngrp, nsg, nhg, sec_count[0],
           sec_count[1], sec_count[2], bad_size, bad_perm, bad_pad, bad_record, bad_bound, bad_flat_lo, bad_height,
           accepted, unsafe, sphere_missed, miss[0], miss[1], miss[2]);
    const char *lname[3] = {"block", "group", "super"};
    for (int lv = 0; lv < 3; ++lv)
        printf("\"%s_failed\": %ld, \"%s_passed\": %ld, \"%s_failed_flat\": %ld, \"%s_passed_flat\": %ld, ", lname[lv],
               walk[lv][0][0], lname[lv], walk[lv][0][1], lname[lv], walk[lv][1][0], lname[lv], walk[lv][1][1]);
    for (int lv = 0; lv < 3; ++lv) printf("\"%s_failed_padding\": %ld, ", lname[lv], pad_failed[lv]);
    printf("\"padding_passed\": %ld, \"half_only_failed\": %ld, \"blocks_stepped\": %ld, \"list_entries\": %ld, "
           "\"rays_over_24_blocks\": %ld, \"rays_over_24_entries\": %ld, \"failures\": %ld}\n",
           pad_passed, half_only, blocks_stepped, entries, rays_over_24_blocks, rays_over_24_entries, failures);
    return failures ? 1 : 0;
}
