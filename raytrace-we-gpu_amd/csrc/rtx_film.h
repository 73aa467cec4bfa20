// rtx_film.h — the host-side rules of film queries (include/rtx.h
// rtx_trace_film, rtx_film_from_frame, rtx_film_camera): a film record's
// layout, the entry point's argument rules, the launch's index arithmetic and
// the two record generators. HIP-free: the host (rtx_host.cpp, rtx_api.hip),
// the kernel (rtx_kernels.hip k_film) and the CPU checker
// (tests/film_check.cpp) run this one text.
//
// A film query is a pixel of a frame of its own: the record carries the
// frame's origin, lower-left corner, horizontal and vertical rows, the pixel's
// (fx, fy) and the seed of its RNG chain; img_w and img_h are per call. Every
// sample starts as the render's start_sample does on those values (two hash2
// draws, u and v, get_ray, the thin lens when the record has one), so query i
// with fx = (float)x, fy = (float)y and seed = rtx_path_seed(x, y, f) is pixel
// (x, y) of rtx_render_sum in that frame, and the CPU oracle's
// render_rows_linear computes it (tests/film_cases.py).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rtx_paths.h"

namespace rtx {

// A film record is four float4: (o.xyz, seed), (L.xyz, tag), (H.xyz, fx),
// (V.xyz, fy); with kFilmLens two more: (lens_u.xyz, lens_r), (lens_v.xyz,
// reserved). o and seed sit where a path query's do.
constexpr uint32_t kFilmBytes = 64u;
constexpr uint32_t kFilmLensBytes = 96u;
constexpr uint32_t kFilmO = 0u;       // float index of o[0]
constexpr uint32_t kFilmSeed = 3u;    // ... of seed
constexpr uint32_t kFilmL = 4u;       // ... of lower_left[0]
constexpr uint32_t kFilmTag = 7u;     // ... of tag (the caller's, unread)
constexpr uint32_t kFilmH = 8u;       // ... of horizontal[0]
constexpr uint32_t kFilmFx = 11u;     // ... of fx
constexpr uint32_t kFilmV = 12u;      // ... of vertical[0]
constexpr uint32_t kFilmFy = 15u;     // ... of fy
constexpr uint32_t kFilmLensU = 16u;  // ... of lens_u[0]
constexpr uint32_t kFilmLensR = 19u;  // ... of lens_r
constexpr uint32_t kFilmLensV = 20u;  // ... of lens_v[0]
constexpr uint32_t kFilmReserved = 23u;

constexpr uint32_t kFilmLens = 4u;  // = RTX_FILM_LENS, beside kPathsLambertGuard and kPathsContinue
constexpr uint32_t kFilmFlagMask = kPathsFlagMask | kFilmLens;
// `order`: RTX_CAST_ORDER_AUTO (0, = GIVEN), _GIVEN (1), RTX_PATHS_ORDER_COST (3).
// _COHERENT (2) is refused: its key pass reads a direction where a film record holds L.
constexpr uint32_t kFilmOrderAuto = 0u, kFilmOrderGiven = 1u, kFilmOrderCoherent = 2u;

// What rtx_trace_film refuses before it looks at the context, in the order it
// tests them (a null ctx comes before all of these): rtx_trace_paths' rules.
enum FilmArg : int {
    kFilmArgOk = 0,
    kFilmArgQueries,  // n > 0 with d_queries NULL
    kFilmArgResults,  // n > 0 with d_results NULL
    kFilmArgSamples,  // samples == 0
    kFilmArgFlags,    // a bit outside kFilmFlagMask
    kFilmArgOrder,    // COHERENT, or above kPathsOrderCost
};
RTX_PATHS_HD FilmArg film_args(bool have_queries, bool have_results, uint32_t n, uint32_t samples, uint32_t flags,
                               uint32_t order) {
    if (n != 0u && !have_queries) return kFilmArgQueries;
    if (n != 0u && !have_results) return kFilmArgResults;
    if (samples == 0u) return kFilmArgSamples;
    if ((flags & ~kFilmFlagMask) != 0u) return kFilmArgFlags;
    if (order == kFilmOrderCoherent || order > kPathsOrderCost) return kFilmArgOrder;
    return kFilmArgOk;
}
// (once the world is known: paths_world, as it stands.)

// float4 per record, and the byte offsets of record i's first float4, of its
// result and of its segment word: 64-bit, so that i * 96 does not wrap.
RTX_PATHS_HD uint32_t film_record_bytes(bool lens) { return lens ? kFilmLensBytes : kFilmBytes; }
RTX_PATHS_HD uint32_t film_record_vec4(bool lens) { return film_record_bytes(lens) / 16u; }
RTX_PATHS_HD uint64_t film_query_offset(uint32_t i, bool lens) { return (uint64_t)i * film_record_bytes(lens); }
RTX_PATHS_HD uint64_t film_query_vec4(uint32_t i, bool lens) { return (uint64_t)i * film_record_vec4(lens); }
RTX_PATHS_HD uint64_t film_result_offset(uint32_t i) { return paths_result_offset(i); }
RTX_PATHS_HD uint64_t film_segment_offset(uint32_t i) { return paths_segment_offset(i); }

// ---- the generators (host) ------------------------------------------------------
// What rtx_film_from_frame refuses, in the order it tests them.
enum FilmFrame : int {
    kFilmFrameOk = 0,
    kFilmFrameNull,       // a null frame, pixel list (n > 0), record buffer or dimension pointer
    kFilmFrameRng,        // a per-sample-RNG frame: a film query runs the chain
    kFilmFrameLens,       // lens == 0 and the frame's lens radius > 0
    kFilmFramePixel,      // some x >= width or y >= height
};

// The records of the listed pixels of a frame, values copied: f is the frame's
// 24 floats in rtx_frame's order of origin, horizontal, vertical, lower_left
// (4 each), lens_u, lens_v (4 each). out: n records of film_record_bytes(lens).
inline FilmFrame film_from_frame(const float origin[4], const float horizontal[4], const float vertical[4],
                                 const float lower_left[4], const float lens_u[4], const float lens_v[4],
                                 uint32_t width, uint32_t height, uint32_t rng_mode, const uint32_t *xs,
                                 const uint32_t *ys, uint32_t n, uint32_t frame_index, void *out, bool lens) {
    if (!origin || !horizontal || !vertical || !lower_left || !lens_u || !lens_v) return kFilmFrameNull;
    if (n != 0u && (!xs || !ys || !out)) return kFilmFrameNull;
    if (rng_mode != 0u) return kFilmFrameRng;
    if (!lens && lens_u[3] > 0.0f) return kFilmFrameLens;
    for (uint32_t i = 0; i < n; ++i)
        if (xs[i] >= width || ys[i] >= height) return kFilmFramePixel;
    unsigned char *dst = static_cast<unsigned char *>(out);
    for (uint32_t i = 0; i < n; ++i) {
        float r[24];
        const uint32_t tag = 0u, reserved = 0u;
        memcpy(r + kFilmO, origin, 12);
        r[kFilmSeed] = path_seed(xs[i], ys[i], frame_index);
        memcpy(r + kFilmL, lower_left, 12);
        memcpy(r + kFilmTag, &tag, 4);
        memcpy(r + kFilmH, horizontal, 12);
        r[kFilmFx] = (float)xs[i];
        memcpy(r + kFilmV, vertical, 12);
        r[kFilmFy] = (float)ys[i];
        memcpy(r + kFilmLensU, lens_u, 16);  // (lens_u.xyz, lens_r)
        memcpy(r + kFilmLensV, lens_v, 12);
        memcpy(r + kFilmReserved, &reserved, 4);
        memcpy(dst + film_query_offset(i, lens), r, film_record_bytes(lens));
    }
    return kFilmFrameOk;
}

// The camera models of rtx_film_camera: unit-form records (fx = fy = 0, to be
// traced with img_w = img_h = 2), one per pixel, row 0 at the bottom.
constexpr int kFilmEquirect = 0;  // = RTX_FILM_EQUIRECT
constexpr int kFilmFisheye = 1;   // = RTX_FILM_FISHEYE
enum FilmCamera : int {
    kFilmCameraOk = 0,
    kFilmCameraNull,   // a null from, at, vup or record buffer
    kFilmCameraModel,  // an unknown model
    kFilmCameraSize,   // width or height 0, or width * height >= 2^32
    kFilmCameraFov,    // fisheye: !(0 < fov <= 360)
    kFilmCameraBasis,  // from == at, or vup parallel to the view direction (or a non-finite input)
};

struct FilmBasis {
    double u[3], v[3], w[3];  // right, up, forward (unit, orthogonal)
};
// The model's unit direction at pixel corner (cx, cy), cx in 0 .. width, cy in
// 0 .. height, in double. Returns false outside a fisheye's image circle.
//   equirect: longitude lon = (cx / width - 0.5) * 2 pi over the width (0 at
//             the centre: forward; positive to the right), latitude lat =
//             (cy / height - 0.5) * pi over the height (row 0 at the bottom);
//             dir = cos(lat) sin(lon) u + sin(lat) v + cos(lat) cos(lon) w.
//   fisheye:  equidistant. (px, py) = (cx - width / 2, cy - height / 2) / (min(width,
//             height) / 2), r = |(px, py)|; outside for r > 1; theta = r * fov / 2,
//             dir = sin(theta) (px u + py v) / r + cos(theta) w (r = 0: forward).
inline bool film_camera_dir(int model, const FilmBasis &B, double fov_deg, uint32_t width, uint32_t height, double cx,
                            double cy, double d[3]) {
    const double kPi = 3.14159265358979323846;
    double a, b, c;  // along u, v, w
    if (model == kFilmEquirect) {
        const double lon = (cx / (double)width - 0.5) * (2.0 * kPi);
        const double lat = (cy / (double)height - 0.5) * kPi;
        a = cos(lat) * sin(lon);
        b = sin(lat);
        c = cos(lat) * cos(lon);
    } else {
        const double half = 0.5 * (double)(width < height ? width : height);
        const double px = (cx - 0.5 * (double)width) / half, py = (cy - 0.5 * (double)height) / half;
        const double r = sqrt(px * px + py * py);
        if (r > 1.0) return false;
        const double theta = r * (fov_deg * kPi / 360.0);
        const double s = r > 0.0 ? sin(theta) / r : 0.0;
        a = s * px;
        b = s * py;
        c = cos(theta);
    }
    for (int k = 0; k < 3; ++k) d[k] = a * B.u[k] + b * B.v[k] + c * B.w[k];
    return true;
}
// w = normalize(at - from), u = normalize(cross(w, vup)), v = cross(u, w).
inline bool film_camera_basis(const float from[3], const float at[3], const float vup[3], FilmBasis &B) {
    double w[3], up[3];
    for (int k = 0; k < 3; ++k) {
        w[k] = (double)at[k] - (double)from[k];
        up[k] = (double)vup[k];
    }
    const double lw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(lw > 0.0) || !(lw <= 1.7976931348623157e308)) return false;
    for (int k = 0; k < 3; ++k) B.w[k] = w[k] / lw;
    double u[3] = {B.w[1] * up[2] - B.w[2] * up[1], B.w[2] * up[0] - B.w[0] * up[2], B.w[0] * up[1] - B.w[1] * up[0]};
    const double lu = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (!(lu > 0.0) || !(lu <= 1.7976931348623157e308)) return false;
    for (int k = 0; k < 3; ++k) B.u[k] = u[k] / lu;
    B.v[0] = B.u[1] * B.w[2] - B.u[2] * B.w[1];
    B.v[1] = B.u[2] * B.w[0] - B.u[0] * B.w[2];
    B.v[2] = B.u[0] * B.w[1] - B.u[1] * B.w[0];
    return true;
}
// The records: with c(x, y) the direction at corner (x, y), L = o + c(x, y),
// H = (c(x + 1, y) - c(x, y)) / 1.1, V = (c(x, y + 1) - c(x, y)) / 1.1, each
// computed in double and rounded once. A pixel with any of its three corners
// outside a fisheye's image circle gets a zero direction: L = o, H = V = 0.
// Such a query traces the zero ray, as rtx_trace_paths does:
// a = 0, every root is NaN, the ray "hits" at t = NaN again and again and each
// sample ends black at the world's depth: its sum is (0, 0, 0), with `depth`
// segments per sample, and the image shows black there. (In a non-empty world;
// in an empty one the sky colour of a zero direction is NaN.)
// out: width * height records of 64 B each.
inline FilmCamera film_camera(int model, const float from[3], const float at[3], const float vup[3], float fov_deg,
                              uint32_t width, uint32_t height, uint32_t frame_index, void *out) {
    if (!from || !at || !vup || !out) return kFilmCameraNull;
    if (model != kFilmEquirect && model != kFilmFisheye) return kFilmCameraModel;
    if (width == 0u || height == 0u || (uint64_t)width * height >= (1ull << 32)) return kFilmCameraSize;
    if (model == kFilmFisheye && !(fov_deg > 0.0f && fov_deg <= 360.0f)) return kFilmCameraFov;
    FilmBasis B;
    if (!film_camera_basis(from, at, vup, B)) return kFilmCameraBasis;
    unsigned char *dst = static_cast<unsigned char *>(out);
    for (uint32_t y = 0; y < height; ++y) {
        for (uint32_t x = 0; x < width; ++x) {
            double c0[3], cx[3], cy[3];
            const bool in = film_camera_dir(model, B, (double)fov_deg, width, height, (double)x, (double)y, c0) &&
                            film_camera_dir(model, B, (double)fov_deg, width, height, (double)x + 1.0, (double)y, cx) &&
                            film_camera_dir(model, B, (double)fov_deg, width, height, (double)x, (double)y + 1.0, cy);
            float r[16];
            const uint32_t tag = 0u;
            for (int k = 0; k < 3; ++k) {
                r[kFilmO + k] = from[k];
                r[kFilmL + k] = in ? (float)((double)from[k] + c0[k]) : from[k];
                r[kFilmH + k] = in ? (float)((cx[k] - c0[k]) / 1.1) : 0.0f;
                r[kFilmV + k] = in ? (float)((cy[k] - c0[k]) / 1.1) : 0.0f;
            }
            r[kFilmSeed] = path_seed(x, y, frame_index);
            memcpy(r + kFilmTag, &tag, 4);
            r[kFilmFx] = 0.0f;
            r[kFilmFy] = 0.0f;
            memcpy(dst + film_query_offset(y * width + x, false), r, kFilmBytes);
        }
    }
    return kFilmCameraOk;
}

}  // namespace rtx
