// hostile_rays.h — the hostile ray classes and degenerate spheres of
// tests/hostile_cases.py for the stand-alone CPU checkers that generate their
// own rays (prefilter_check, grid_check, grid_coop_check, layout_check): a
// checker builds an ordinary ray at a sphere c of its scene and, in its
// hostile mode, hands every few of them to hostile_ray(), which turns it into
// the next class in turn. The point for the checkers is twofold: the claims
// they check (a sphere the reference takes is flagged, marked, walked) must
// hold for these rays too, a NaN discriminant or root counting as taken, and
// the walks' float-to-int conversions must stay defined when a coordinate is
// NaN or infinite (the sanitizer builds of tests/test_hostile_inputs.py).
#pragma once

#include <cmath>

namespace hostile {

constexpr int kClasses = 36;

inline void rescale(float d[3], double len) {
    const double n = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    if (!(n > 0.0)) {
        d[0] = (float)len, d[1] = 0.0f, d[2] = 0.0f;
        return;
    }
    for (int i = 0; i < 3; ++i) d[i] = (float)((double)d[i] / n * len);
}

// (o, d): an ordinary ray, c = (cx, cy, cz, r) a sphere of the scene. Classes:
//  0-17  NaN, +inf, -inf in each of the six components alone
//  18-19 d = (0, 0, 0), d = (-0, -0, -0)
//  20-23 |d| = 1e-19, 1e-20, 1e-23, 3e-39
//  24-28 |d| = 1e10, 1.5e19, 3e19, 1e25, 1e38
//  29-32 |o| = 1e8, 1e20, 1e30, 3e38, aimed at c
//  33    o = c
//  34    o = c + (|r|, 0, 0)
//  35    the same with |d| = 3e19
inline void hostile_ray(int cls, const float *c, float o[3], float d[3]) {
    static const double tiny[4] = {1e-19, 1e-20, 1e-23, 3e-39};
    static const double huge[5] = {1e10, 1.5e19, 3e19, 1e25, 1e38};
    static const double far_o[4] = {1e8, 1e20, 1e30, 3e38};
    cls = ((cls % kClasses) + kClasses) % kClasses;
    if (cls < 18) {
        const float v = cls % 3 == 0 ? NAN : cls % 3 == 1 ? INFINITY : -INFINITY;
        float *p = cls < 9 ? o : d;
        p[(cls / 3) % 3] = v;
    } else if (cls < 20) {
        d[0] = d[1] = d[2] = cls == 18 ? 0.0f : -0.0f;
    } else if (cls < 24) {
        rescale(d, tiny[cls - 20]);
    } else if (cls < 29) {
        rescale(d, huge[cls - 24]);
    } else if (cls < 33) {
        rescale(o, far_o[cls - 29]);
        for (int i = 0; i < 3; ++i) d[i] = c[i] - o[i];
    } else {
        for (int i = 0; i < 3; ++i) o[i] = c[i];
        if (cls >= 34) o[0] = c[0] + std::fabs(c[3]);
        if (cls == 35) rescale(d, 3e19);
    }
}

// Sphere j of a scene made degenerate, kind 0-5 as degenerate_spheres: radius
// 0, -0, negated, 1e-30, concentric with sphere j - 1 (x and z only when
// keep_y: a layer keeps its height), centre and radius on the 1/8 lattice.
inline void degenerate_sphere(float *sph, unsigned j, int kind, bool keep_y) {
    float *s = sph + 4 * (size_t)j;
    switch (kind % 6) {
        case 0: s[3] = 0.0f; break;
        case 1: s[3] = -0.0f; break;
        case 2: s[3] = -s[3]; break;
        case 3: s[3] = 1e-30f; break;
        case 4:
            if (j > 0) {
                s[0] = s[-4], s[2] = s[-2];
                if (!keep_y) s[1] = s[-3];
            }
            break;
        default:
            s[0] = std::round(s[0] * 8.0f) / 8.0f, s[2] = std::round(s[2] * 8.0f) / 8.0f;
            if (!keep_y) s[1] = std::round(s[1] * 8.0f) / 8.0f;
            s[3] = std::floor(std::fabs(s[3]) * 8.0f) / 8.0f + 0.125f;
            break;
    }
}

}  // namespace hostile
