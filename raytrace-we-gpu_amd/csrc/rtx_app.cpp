// rtx_app.cpp — RtxBase / RtxCSApp: the reference's CDx11Base / DxCSApp
// entry-point surface (LoadContent / Update / Render / UnloadContent) over
// the rtx C-ABI. See include/rtx_app.hpp.
#include "../../include/rtx_app.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

namespace rtx {

// Derived classes call Terminate() in their own destructor (UnloadContent
// is virtual); the base only releases a context still held.
RtxBase::~RtxBase() {
    if (m_group) rtx_group_destroy(m_group);
    else if (m_ctx) rtx_destroy(m_ctx);
}

bool RtxBase::Initialize(int hip_device) {
    if (m_ctx) return true;
    if (rtx_create(hip_device, &m_ctx) != RTX_OK) {
        m_error = rtx_last_error();
        m_ctx = nullptr;
        return false;
    }
    return LoadContent();
}

bool RtxBase::Initialize(const std::vector<int> &devices, int gather_mode) {
    if (m_ctx) return true;
    if (rtx_group_create(devices.data(), (uint32_t)devices.size(), gather_mode, &m_group) != RTX_OK) {
        m_error = rtx_last_error();
        m_group = nullptr;
        return false;
    }
    m_ctx = rtx_group_ctx(m_group, 0);
    return LoadContent();
}

void RtxBase::Terminate() {
    if (!m_ctx) return;
    UnloadContent();
    if (m_group) rtx_group_destroy(m_group);  // its members' contexts with it
    else rtx_destroy(m_ctx);
    m_group = nullptr;
    m_ctx = nullptr;
}

RtxCSApp::RtxCSApp(const AppConfig &cfg) : m_cfg(cfg) {}

bool fill_worlddef(const AppConfig &cfg, WorldDefBytes &out) {
    std::memset(&out, 0, sizeof(out));
    float sph[4 * 512], mt[512], mv[4 * 512];
    uint32_t n = 0;
    if (rtx_scene_random_world(cfg.grid_half_extent, 512, sph, mt, mv, &n) != RTX_OK) return false;
    const uint64_t full = 4ull + 4ull * (uint64_t)cfg.grid_half_extent * cfg.grid_half_extent;
    if (full > 512) return false;  // the cbuffer holds 512 spheres (DxCSApp.cpp:67)
    for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 4; ++k) {
            out.spheres[i][k] = sph[4 * i + k];
            out.mat_values[i][k] = mv[4 * i + k];
        }
        out.mat_types[i / 4][i % 4] = mt[i];  // SetFloat4Cmpt(matTypes[i/4], i%4, .)
    }
    out.scene_values[0] = (float)n;  // { count, 50, 60, -1 } (:133)
    out.scene_values[1] = (float)cfg.depth;
    out.scene_values[2] = (float)cfg.spp;
    out.scene_values[3] = -1.0f;
    return true;
}

bool fill_perframe(const AppConfig &cfg, float sample_count, PerFrameBytes &out) {
    std::memset(&out, 0, sizeof(out));
    const float persp[4] = {cfg.vfov, cfg.aspect, cfg.aperture, (float)cfg.width};  // :179
    rtx_frame f{};
    // ComputeViewVals(camPos, camLookAt, upDir, vfov, aspect, aperture, focus_dist) (:488-489)
    if (rtx_camera_look_at(cfg.cam_pos, cfg.cam_look_at, cfg.up, persp[0], persp[1], persp[2], 0.0f, cfg.width,
                           cfg.height, &f) != RTX_OK)
        return false;
    std::memcpy(out.perspective_vals, persp, sizeof(persp));
    const float *rows[4] = {f.origin, f.horizontal, f.vertical, f.lower_left};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out.view_vals[4 * j + i] = rows[i][j];  // XMMatrixTranspose (:60)
    for (int k = 0; k < 4; ++k) out.curr_samples[k] = sample_count;       // (:491-492)
    return true;
}

RtxCSApp::~RtxCSApp() { Terminate(); }

bool RtxCSApp::LoadContent() {
    if (m_cfg.cbuffers) {  // the reference's WorldDef bytes through the adapter
        WorldDefBytes wd;
        rtx_world w{};
        m_spheres.assign(4 * 512, 0.0f);
        m_mat_types.assign(512, 0.0f);
        m_mat_values.assign(4 * 512, 0.0f);
        if (m_cfg.scene != SceneKind::RandomWorld || !fill_worlddef(m_cfg, wd) ||
            rtx_world_from_worlddef(&wd, sizeof(wd), m_spheres.data(), m_mat_types.data(), m_mat_values.data(),
                                    &w) != RTX_OK) {
            m_error = "WorldDef: only random_world scenes of at most 512 spheres fit the cbuffer";
            return m_ok = false;
        }
        m_count = w.count;
        m_depth = w.depth;
        // CreateBuffer(WorldDef, IMMUTABLE) (:393-413)
        if ((m_group ? rtx_group_upload_world(m_group, &w) : rtx_upload_world(m_ctx, &w)) != RTX_OK) {
            m_error = rtx_last_error();
            return m_ok = false;
        }
        return m_ok = true;
    }
    // WorldDef w; WorldDef::random_world(w);  (DxCSApp.cpp:401-402)
    uint32_t cap = m_cfg.scene == SceneKind::PsWorld ? 7 : 4;
    if (m_cfg.scene == SceneKind::RandomWorld) {
        const uint64_t full = 4ull + 4ull * (uint64_t)m_cfg.grid_half_extent * m_cfg.grid_half_extent;
        cap = (uint32_t)std::min<uint64_t>(full, m_cfg.max_spheres ? m_cfg.max_spheres : full);
    }
    m_spheres.assign(4 * (size_t)cap, 0.0f);
    m_mat_types.assign(cap, 0.0f);
    m_mat_values.assign(4 * (size_t)cap, 0.0f);
    int rc = (m_cfg.scene == SceneKind::RandomWorld)
                 ? rtx_scene_random_world(m_cfg.grid_half_extent, cap, m_spheres.data(),
                                          m_mat_types.data(), m_mat_values.data(), &m_count)
                 : (m_cfg.scene == SceneKind::PsWorld)
                       ? rtx_scene_ps_world(m_spheres.data(), m_mat_types.data(), m_mat_values.data(), &m_count)
                       : rtx_scene_test_world(m_spheres.data(), m_mat_types.data(), m_mat_values.data(),
                                              &m_count);
    if (rc != RTX_OK) {
        m_error = "scene generation failed";
        return m_ok = false;
    }
    rtx_world w{};
    w.count = m_count;
    w.depth = m_cfg.depth;
    w.spp = m_cfg.spp;
    m_depth = w.depth;
    w.spheres = m_spheres.data();
    w.mat_types = m_mat_types.data();
    w.mat_values = m_mat_values.data();
    // CreateBuffer(WorldDef, IMMUTABLE)  (DxCSApp.cpp:393-413)
    if ((m_group ? rtx_group_upload_world(m_group, &w) : rtx_upload_world(m_ctx, &w)) != RTX_OK) {
        m_error = rtx_last_error();
        return m_ok = false;
    }
    return m_ok = true;
}

void RtxCSApp::UnloadContent() {
    // Device resources belong to the context; RtxBase::Terminate destroys it.
    m_spheres.clear();
    m_mat_types.clear();
    m_mat_values.clear();
}

void RtxCSApp::Update() {
    // focus_dist = |camPos - camLookAt|; ComputeViewVals; sampleCount++
    // (DxCSApp.cpp:488-492), then the PerFrame upload (:494-496).
    int rc;
    if (m_cfg.cbuffers) {  // the reference's PerFrame bytes through the adapter
        PerFrameBytes pf;
        rc = fill_perframe(m_cfg, (float)(m_frame_count + 1), pf)
                 ? rtx_frame_from_perframe(&pf, sizeof(pf), m_cfg.width, m_cfg.height, &m_frame)
                 : RTX_ERR_INVALID;
    } else if (m_cfg.simple_camera)
        rc = rtx_camera_simple(m_cfg.width, m_cfg.height, &m_frame);
    else
        rc = rtx_camera_look_at(m_cfg.cam_pos, m_cfg.cam_look_at, m_cfg.up, m_cfg.vfov, m_cfg.aspect,
                                m_cfg.aperture, m_cfg.focus_dist, m_cfg.width, m_cfg.height, &m_frame);
    m_frame.rng_mode = m_cfg.rng_mode;
    m_frame.flags = m_cfg.lambert_guard ? RTX_FRAME_LAMBERT_GUARD : 0u;
    if (rc == RTX_OK && m_cfg.lens_aperture > 0.0f) rc = rtx_camera_set_aperture(&m_frame, m_cfg.lens_aperture);
    ++m_frame_count;
    if (rc != RTX_OK || (m_group ? rtx_group_set_frame(m_group, &m_frame) : rtx_set_frame(m_ctx, &m_frame)) != RTX_OK) {
        m_error = rtx_last_error();
        m_ok = false;
    }
}

void RtxCSApp::Render() {
    // Dispatch(32,32,1)  (DxCSApp.cpp:524)
    if (!m_ok) return;
    if ((m_group ? rtx_group_render(m_group, m_cfg.tile_rows) : rtx_render(m_ctx)) != RTX_OK) {
        m_error = rtx_last_error();
        m_ok = false;
    }
}

bool RtxCSApp::Accumulate(uint32_t frames, bool reset) {
    if (!m_ok) return false;
    int rc = RTX_OK;
    if (m_group) {
        rc = rtx_group_accumulate(m_group, frames, reset ? 1 : 0);
    } else {
        if (frames == 0) {  // refused like the group's
            m_error = "Accumulate: frames is 0";
            return m_ok = false;
        }
        for (uint32_t k = 0; k < frames && rc == RTX_OK; ++k) rc = rtx_accumulate(m_ctx, (reset && k == 0) ? 1 : 0);
    }
    if (rc != RTX_OK) {
        m_error = rtx_last_error();
        m_ok = false;
    }
    return m_ok;
}

bool RtxCSApp::Refine(uint32_t samples, bool reset) {
    if (!m_ok) return false;
    if ((m_group ? rtx_group_refine(m_group, samples, m_cfg.tile_rows, reset ? 1 : 0)
                 : rtx_refine(m_ctx, samples, reset ? 1 : 0)) != RTX_OK) {
        m_error = rtx_last_error();
        m_ok = false;
    }
    return m_ok;
}

bool RtxCSApp::RefineAdaptive(uint32_t samples, float threshold, uint32_t max_samples, bool reset, uint32_t *active) {
    if (!m_ok) return false;
    if ((m_group ? rtx_group_refine_adaptive(m_group, samples, threshold, max_samples, m_cfg.tile_rows, reset ? 1 : 0,
                                             active)
                 : rtx_refine_adaptive(m_ctx, samples, threshold, max_samples, reset ? 1 : 0, active)) != RTX_OK) {
        m_error = rtx_last_error();
        m_ok = false;
    }
    return m_ok;
}

bool RtxCSApp::SetRefineKeys(int mode) {
    if (!m_ok) return false;
    if (!m_ctx) {
        m_error = "SetRefineKeys: not initialized";
        return false;
    }
    // with a group: every member's launches
    const uint32_t members = m_group ? rtx_group_size(m_group) : 1u;
    for (uint32_t m = 0; m < members; ++m) {
        if (rtx_refine_set_keys(m_group ? rtx_group_ctx(m_group, m) : m_ctx, mode) != RTX_OK) {
            m_error = rtx_last_error();
            return false;
        }
    }
    return true;
}

bool RtxCSApp::Features(std::vector<float> &geom, std::vector<float> &surf) {
    if (!m_ok) return false;
    const size_t bytes = 4 * (size_t)m_frame.width * m_frame.height * sizeof(float);
    void *d[2] = {nullptr, nullptr};
    bool ok = rtx_alloc(m_ctx, bytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, bytes, &d[1]) == RTX_OK &&
              rtx_features(m_ctx, d[0], d[1]) == RTX_OK;
    if (ok) {
        geom.resize(bytes / sizeof(float));
        surf.resize(bytes / sizeof(float));
        ok = rtx_copy_to_host(m_ctx, geom.data(), d[0], bytes) == RTX_OK &&
             rtx_copy_to_host(m_ctx, surf.data(), d[1], bytes) == RTX_OK;
    }
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

bool RtxCSApp::Cast(const std::vector<rtx_ray> &rays, std::vector<rtx_ray_hit> *hits, int order, float t_min) {
    if (!m_ok) return false;
    if (!hits) {
        m_error = "Cast: hits is NULL";
        return false;
    }
    hits->resize(rays.size());
    if (rays.size() > 0xffffffffull) {
        m_error = "Cast: more than 2^32 - 1 rays";
        return false;
    }
    const uint32_t n = (uint32_t)rays.size();
    const size_t bytes = (size_t)n * sizeof(rtx_ray);
    void *d[2] = {nullptr, nullptr};
    bool ok = n == 0 || (rtx_alloc(m_ctx, bytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, bytes, &d[1]) == RTX_OK &&
                         rtx_copy_to_device(m_ctx, d[0], rays.data(), bytes) == RTX_OK);
    ok = ok && rtx_cast_rays(m_ctx, d[0], n, t_min, (uint32_t)order, d[1], nullptr) == RTX_OK;
    if (ok && n != 0) ok = rtx_copy_to_host(m_ctx, hits->data(), d[1], bytes) == RTX_OK;
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

int RtxCSApp::CastLastOrder() const { return m_ctx ? rtx_cast_last_order(m_ctx) : RTX_CAST_ORDER_GIVEN; }

bool RtxCSApp::TracePaths(const std::vector<rtx_path_query> &queries, uint32_t samples,
                          std::vector<rtx_path_result> *results, uint32_t flags, int order,
                          std::vector<uint32_t> *segments) {
    if (!m_ok) return false;
    if (!results) {
        m_error = "TracePaths: results is NULL";
        return false;
    }
    if (queries.size() > 0xffffffffull) {
        m_error = "TracePaths: more than 2^32 - 1 queries";
        return false;
    }
    const bool cont = (flags & RTX_PATHS_CONTINUE) != 0u;
    if (cont && results->size() != queries.size()) {
        m_error = "TracePaths: RTX_PATHS_CONTINUE needs one record per query to continue from";
        return false;
    }
    results->resize(queries.size());
    if (segments) segments->resize(queries.size());
    const uint32_t n = (uint32_t)queries.size();
    const size_t qbytes = (size_t)n * sizeof(rtx_path_query), rbytes = (size_t)n * sizeof(rtx_path_result);
    const size_t sbytes = (size_t)n * sizeof(uint32_t);
    void *d[3] = {nullptr, nullptr, nullptr};
    bool ok = n == 0 || (rtx_alloc(m_ctx, qbytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, rbytes, &d[1]) == RTX_OK &&
                         (!segments || rtx_alloc(m_ctx, sbytes, &d[2]) == RTX_OK) &&
                         rtx_copy_to_device(m_ctx, d[0], queries.data(), qbytes) == RTX_OK &&
                         (!cont || rtx_copy_to_device(m_ctx, d[1], results->data(), rbytes) == RTX_OK));
    ok = ok && rtx_trace_paths(m_ctx, d[0], n, samples, flags, (uint32_t)order, d[1], d[2]) == RTX_OK;
    if (ok && n != 0) ok = rtx_copy_to_host(m_ctx, results->data(), d[1], rbytes) == RTX_OK;
    if (ok && n != 0 && segments) ok = rtx_copy_to_host(m_ctx, segments->data(), d[2], sbytes) == RTX_OK;
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

bool RtxCSApp::TraceFilm(const void *queries, size_t count, uint32_t samples, float img_w, float img_h,
                         std::vector<rtx_path_result> *results, uint32_t flags, int order,
                         std::vector<uint32_t> *segments) {
    if (!m_ok) return false;
    if (!results || (count != 0 && !queries)) {
        m_error = "TraceFilm: queries or results is NULL";
        return false;
    }
    if (count > 0xffffffffull) {
        m_error = "TraceFilm: more than 2^32 - 1 queries";
        return false;
    }
    const bool cont = (flags & RTX_PATHS_CONTINUE) != 0u;
    if (cont && results->size() != count) {
        m_error = "TraceFilm: RTX_PATHS_CONTINUE needs one record per query to continue from";
        return false;
    }
    results->resize(count);
    if (segments) segments->resize(count);
    const uint32_t n = (uint32_t)count;
    const size_t rec = (flags & RTX_FILM_LENS) != 0u ? sizeof(rtx_film_lens_query) : sizeof(rtx_film_query);
    const size_t qbytes = (size_t)n * rec, rbytes = (size_t)n * sizeof(rtx_path_result);
    const size_t sbytes = (size_t)n * sizeof(uint32_t);
    void *d[3] = {nullptr, nullptr, nullptr};
    bool ok = n == 0 || (rtx_alloc(m_ctx, qbytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, rbytes, &d[1]) == RTX_OK &&
                         (!segments || rtx_alloc(m_ctx, sbytes, &d[2]) == RTX_OK) &&
                         rtx_copy_to_device(m_ctx, d[0], queries, qbytes) == RTX_OK &&
                         (!cont || rtx_copy_to_device(m_ctx, d[1], results->data(), rbytes) == RTX_OK));
    ok = ok && rtx_trace_film(m_ctx, d[0], n, samples, img_w, img_h, flags, (uint32_t)order, d[1], d[2]) == RTX_OK;
    if (ok && n != 0) ok = rtx_copy_to_host(m_ctx, results->data(), d[1], rbytes) == RTX_OK;
    if (ok && n != 0 && segments) ok = rtx_copy_to_host(m_ctx, segments->data(), d[2], sbytes) == RTX_OK;
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

int RtxCSApp::FilmLastOrder() const { return m_ctx ? rtx_film_last_order(m_ctx) : RTX_CAST_ORDER_GIVEN; }

bool RtxCSApp::FilmImage(const std::vector<rtx_path_result> &results, uint32_t samples, std::vector<float> *rgba) {
    if (!m_ok) return false;
    if (!rgba || results.empty() || samples == 0u) {
        m_error = "FilmImage: no records, no samples or rgba is NULL";
        return false;
    }
    const size_t n = results.size(), bytes = n * sizeof(rtx_path_result);
    rgba->assign(4 * n, 0.0f);
    void *d[3] = {nullptr, nullptr, nullptr};  // accumulator (zeroed), sums, image
    bool ok = rtx_alloc(m_ctx, bytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, bytes, &d[1]) == RTX_OK &&
              rtx_alloc(m_ctx, bytes, &d[2]) == RTX_OK &&
              rtx_copy_to_device(m_ctx, d[0], rgba->data(), bytes) == RTX_OK &&
              rtx_copy_to_device(m_ctx, d[1], results.data(), bytes) == RTX_OK &&
              rtx_fold_frames(m_ctx, d[0], d[1], 1, n, n, samples, d[2]) == RTX_OK &&
              rtx_copy_to_host(m_ctx, rgba->data(), d[2], bytes) == RTX_OK;
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

bool RtxCSApp::TracePathsKeyed(const std::vector<rtx_path_query> &queries, uint32_t samples,
                               std::vector<rtx_path_result> *results, uint32_t flags,
                               const std::vector<uint32_t> *keys, uint32_t probe, std::vector<uint32_t> *segments) {
    if (!m_ok) return false;
    if (!results) {
        m_error = "TracePathsKeyed: results is NULL";
        return false;
    }
    if (queries.size() > 0xffffffffull) {
        m_error = "TracePathsKeyed: more than 2^32 - 1 queries";
        return false;
    }
    if (keys && keys->size() != queries.size()) {
        m_error = "TracePathsKeyed: one key per query";
        return false;
    }
    const bool cont = (flags & RTX_PATHS_CONTINUE) != 0u;
    if (cont && results->size() != queries.size()) {
        m_error = "TracePathsKeyed: RTX_PATHS_CONTINUE needs one record per query to continue from";
        return false;
    }
    results->resize(queries.size());
    if (segments) segments->resize(queries.size());
    const uint32_t n = (uint32_t)queries.size();
    const size_t qbytes = (size_t)n * sizeof(rtx_path_query), rbytes = (size_t)n * sizeof(rtx_path_result);
    const size_t sbytes = (size_t)n * sizeof(uint32_t);
    void *d[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = n == 0 || (rtx_alloc(m_ctx, qbytes, &d[0]) == RTX_OK && rtx_alloc(m_ctx, rbytes, &d[1]) == RTX_OK &&
                         (!segments || rtx_alloc(m_ctx, sbytes, &d[2]) == RTX_OK) &&
                         (!keys || (rtx_alloc(m_ctx, sbytes, &d[3]) == RTX_OK &&
                                    rtx_copy_to_device(m_ctx, d[3], keys->data(), sbytes) == RTX_OK)) &&
                         rtx_copy_to_device(m_ctx, d[0], queries.data(), qbytes) == RTX_OK &&
                         (!cont || rtx_copy_to_device(m_ctx, d[1], results->data(), rbytes) == RTX_OK));
    // (an empty batch with keys: any non-null pointer says "keys given", and nothing reads it)
    const void *kp = keys ? (n != 0 ? d[3] : static_cast<const void *>(keys)) : nullptr;
    ok = ok && rtx_trace_paths_keyed(m_ctx, d[0], n, samples, flags, kp, probe, d[1], d[2]) == RTX_OK;
    if (ok && n != 0) ok = rtx_copy_to_host(m_ctx, results->data(), d[1], rbytes) == RTX_OK;
    if (ok && n != 0 && segments) ok = rtx_copy_to_host(m_ctx, segments->data(), d[2], sbytes) == RTX_OK;
    if (!ok) m_error = rtx_last_error();
    for (void *p : d)
        if (p) rtx_free(m_ctx, p);
    return ok;
}

int RtxCSApp::PathsLastOrder() const { return m_ctx ? rtx_paths_last_order(m_ctx) : RTX_CAST_ORDER_GIVEN; }

bool RtxCSApp::Pick(uint32_t x, uint32_t y, rtx_hit *out) {
    if (!m_ok) return false;
    if (rtx_pick(m_ctx, x, y, out) != RTX_OK) {
        m_error = rtx_last_error();
        return false;
    }
    return true;
}

bool RtxCSApp::FocusAt(uint32_t x, uint32_t y, float aperture) {
    if (!m_ok) return false;
    if (m_cfg.simple_camera || m_cfg.cbuffers) {
        m_error = "FocusAt: needs the look-at camera (not the simple camera or the cbuffer path)";
        return false;
    }
    rtx_hit h{};
    if (!Pick(x, y, &h)) return false;
    if (!h.hit) {
        m_error = "FocusAt: nothing under pixel (" + std::to_string(x) + ", " + std::to_string(y) + ")";
        return false;
    }
    // the hit's distance along the view axis: the focus plane is normal to it
    float w[3], len2 = 0.0f, along = 0.0f;
    for (int k = 0; k < 3; ++k) {
        w[k] = m_cfg.cam_look_at[k] - m_cfg.cam_pos[k];
        len2 += w[k] * w[k];
    }
    const float len = std::sqrt(len2);
    for (int k = 0; k < 3; ++k) along += (h.p[k] - m_cfg.cam_pos[k]) * (w[k] / len);
    if (!(along > 0.0f) || !(aperture >= 0.0f)) {
        m_error = "FocusAt: no focus plane in front of the camera, or a negative aperture";
        return false;
    }
    m_cfg.focus_dist = along;
    m_cfg.lens_aperture = aperture;
    Update();
    return m_ok;
}

bool RtxCSApp::RefineMasked(uint32_t samples, const std::vector<uint32_t> &ids, uint32_t grow, uint32_t max_samples,
                            uint32_t *active, uint32_t *mask_pixels) {
    if (!m_ok) return false;
    if (m_group) {
        m_error = "RefineMasked: masked refinement runs on one context over the whole frame, not on a group";
        return false;
    }
    const size_t px = (size_t)m_frame.width * m_frame.height;
    void *d_surf = nullptr, *d_mask = nullptr;
    uint32_t set = 0;
    const bool ok = rtx_alloc(m_ctx, px * 4 * sizeof(float), &d_surf) == RTX_OK && rtx_alloc(m_ctx, px, &d_mask) == RTX_OK &&
                    rtx_features(m_ctx, nullptr, d_surf) == RTX_OK &&
                    rtx_mask_from_ids(m_ctx, d_surf, ids.data(), (uint32_t)ids.size(), grow, d_mask, &set) == RTX_OK &&
                    rtx_refine_masked(m_ctx, samples, d_mask, max_samples, active) == RTX_OK &&
                    rtx_sync(m_ctx) == RTX_OK;  // the mask is read by the launch: freed after it
    if (!ok) m_error = rtx_last_error();
    if (mask_pixels) *mask_pixels = set;
    if (d_surf) rtx_free(m_ctx, d_surf);
    if (d_mask) rtx_free(m_ctx, d_mask);
    return ok;
}

uint32_t RtxCSApp::RefinedSamples() const {
    return m_group ? rtx_group_refined_samples(m_group) : rtx_refined_samples(m_ctx);
}

bool RtxCSApp::SaveState(const std::string &path) {
    if (!m_ctx) {
        m_error = "SaveState: not initialized";
        return false;
    }
    ChainStateHeader h;
    h.width = m_frame.width;
    h.height = m_frame.height;
    h.samples = RefinedSamples();
    h.world_hash = chain_world_hash(m_count, m_depth, m_spheres.data(), m_mat_types.data(), m_mat_values.data());
    h.frame_hash = chain_frame_hash(m_frame);
    {
        // the file holds one N for the frame: after adaptive steps (RefineAdaptive)
        // the per-pixel counts must still be uniform
        std::vector<uint32_t> counts((size_t)h.width * h.height);
        const size_t bytes = counts.size() * sizeof(uint32_t);
        if ((m_group ? rtx_group_refine_counts(m_group, counts.data(), bytes)
                     : rtx_refine_counts(m_ctx, counts.data(), bytes)) != RTX_OK) {
            m_error = rtx_last_error();
            return false;
        }
        if (*std::min_element(counts.begin(), counts.end()) != *std::max_element(counts.begin(), counts.end())) {
            m_error = "SaveState: the per-pixel sample counts differ after adaptive steps, and the state file holds "
                      "one count for the frame (a checkpoint of adaptive state is not supported)";
            return false;
        }
    }
    // a group's parts come back as the one whole-frame state a context exports
    std::vector<float> st(4 * (size_t)h.width * h.height);
    if ((m_group ? rtx_group_refine_export(m_group, st.data(), st.size() * sizeof(float))
                 : rtx_refine_export(m_ctx, st.data(), st.size() * sizeof(float))) != RTX_OK) {
        m_error = rtx_last_error();
        return false;
    }
    if (!write_chain_state(path, h, st.data())) {
        m_error = "SaveState: cannot write " + path;
        return false;
    }
    return true;
}

bool RtxCSApp::LoadState(const std::string &path) {
    if (!m_ctx) {
        m_error = "LoadState: not initialized";
        return false;
    }
    ChainStateHeader want;
    want.width = m_frame.width;
    want.height = m_frame.height;
    want.world_hash = chain_world_hash(m_count, m_depth, m_spheres.data(), m_mat_types.data(), m_mat_values.data());
    want.frame_hash = chain_frame_hash(m_frame);
    std::vector<float> st;
    uint32_t samples = 0;
    if (!read_chain_state(path, want, st, samples, m_error)) return false;
    if ((m_group ? rtx_group_refine_import(m_group, m_cfg.tile_rows, st.data(), st.size() * sizeof(float), samples)
                 : rtx_refine_import(m_ctx, st.data(), st.size() * sizeof(float), samples)) != RTX_OK) {
        m_error = rtx_last_error();
        return false;
    }
    return true;
}

bool RtxCSApp::Download(std::vector<float> &rgba) {
    rgba.resize(4 * (size_t)m_cfg.width * m_cfg.height);
    const size_t bytes = rgba.size() * sizeof(float);
    if ((m_group ? rtx_group_download(m_group, rgba.data(), bytes) : rtx_download(m_ctx, rgba.data(), bytes)) != RTX_OK) {
        m_error = rtx_last_error();
        return false;
    }
    return true;
}

bool write_pfm(const std::string &path, const float *rgba, uint32_t w, uint32_t h) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);  // negative scale: little endian
    std::vector<float> row(3 * (size_t)w);
    bool ok = true;
    for (uint32_t y = 0; y < h && ok; ++y) {  // PFM rows run bottom-to-top
        for (uint32_t x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) row[3 * x + c] = rgba[4 * ((size_t)y * w + x) + c];
        ok = std::fwrite(row.data(), sizeof(float), row.size(), f) == row.size();
    }
    return std::fclose(f) == 0 && ok;
}

bool write_ppm(const std::string &path, const float *rgba, uint32_t w, uint32_t h) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", w, h);
    std::vector<unsigned char> row(3 * (size_t)w);
    bool ok = true;
    for (uint32_t yy = 0; yy < h && ok; ++yy) {
        const uint32_t y = h - 1 - yy;  // top row first
        for (uint32_t x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                float v = rgba[4 * ((size_t)y * w + x) + c];
                v = std::isnan(v) ? 0.0f : std::min(1.0f, std::max(0.0f, v));
                row[3 * x + c] = (unsigned char)(255.999f * v);  // Color.h:6-11 scaling
            }
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    return std::fclose(f) == 0 && ok;
}

namespace {

constexpr char kChainMagic[8] = {'R', 'T', 'X', 'C', 'H', 'A', 'I', 'N'};
constexpr size_t kChainHeaderBytes = 8 + 4 * 4 + 2 * 8;

uint64_t fnv1a(uint64_t h, const void *data, size_t n) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

void put_le(unsigned char *p, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) p[i] = (unsigned char)(v >> (8 * i));
}
uint64_t get_le(const unsigned char *p, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
// float <-> little-endian bytes, whatever the host's order
void put_f32(unsigned char *p, float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    put_le(p, u, 4);
}
float get_f32(const unsigned char *p) {
    const uint32_t u = (uint32_t)get_le(p, 4);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
std::string hex64(uint64_t v) {
    char b[24];
    std::snprintf(b, sizeof b, "%016llx", (unsigned long long)v);
    return b;
}

}  // namespace

uint64_t chain_world_hash(uint32_t count, uint32_t depth, const float *spheres, const float *mat_types,
                          const float *mat_values) {
    unsigned char head[8];
    put_le(head, count, 4);
    put_le(head + 4, depth, 4);
    uint64_t h = fnv1a(kFnvBasis, head, sizeof head);
    unsigned char b[4];
    const float *arr[3] = {spheres, mat_types, mat_values};
    const size_t len[3] = {4 * (size_t)count, count, 4 * (size_t)count};
    for (int a = 0; a < 3; ++a)
        for (size_t i = 0; i < len[a]; ++i) {
            put_f32(b, arr[a][i]);
            h = fnv1a(h, b, 4);
        }
    return h;
}

uint64_t chain_frame_hash(const rtx_frame &frame) {
    // every field of rtx_frame is a 4-byte value and the struct has no
    // padding: hashed word by word in little-endian order
    static_assert(sizeof(rtx_frame) % 4 == 0, "rtx_frame is a sequence of 4-byte fields");
    uint64_t h = kFnvBasis;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&frame);
    for (size_t i = 0; i < sizeof(rtx_frame); i += 4) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        unsigned char b[4];
        put_le(b, u, 4);
        h = fnv1a(h, b, 4);
    }
    return h;
}

bool write_chain_state(const std::string &path, const ChainStateHeader &hdr, const float *state) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    unsigned char head[kChainHeaderBytes];
    std::memcpy(head, kChainMagic, 8);
    put_le(head + 8, kChainStateVersion, 4);
    put_le(head + 12, hdr.width, 4);
    put_le(head + 16, hdr.height, 4);
    put_le(head + 20, hdr.samples, 4);
    put_le(head + 24, hdr.world_hash, 8);
    put_le(head + 32, hdr.frame_hash, 8);
    bool ok = std::fwrite(head, 1, sizeof head, f) == sizeof head;
    std::vector<unsigned char> row(16 * (size_t)hdr.width);
    for (uint32_t y = 0; y < hdr.height && ok; ++y) {
        for (size_t i = 0; i < 4 * (size_t)hdr.width; ++i) put_f32(&row[4 * i], state[4 * (size_t)y * hdr.width + i]);
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    return std::fclose(f) == 0 && ok;
}

bool read_chain_state(const std::string &path, const ChainStateHeader &expect, std::vector<float> &state,
                      uint32_t &samples, std::string &error) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        error = "chain state: cannot open " + path;
        return false;
    }
    auto refuse = [&](const std::string &why) {
        std::fclose(f);
        error = "chain state " + path + ": " + why;
        return false;
    };
    unsigned char head[kChainHeaderBytes];
    if (std::fread(head, 1, sizeof head, f) != sizeof head) return refuse("truncated header");
    if (std::memcmp(head, kChainMagic, 8) != 0) return refuse("wrong magic (not a chain-state file)");
    const uint32_t version = (uint32_t)get_le(head + 8, 4);
    if (version != kChainStateVersion)
        return refuse("format version " + std::to_string(version) + ", this build reads " +
                      std::to_string(kChainStateVersion));
    const uint32_t w = (uint32_t)get_le(head + 12, 4), h = (uint32_t)get_le(head + 16, 4);
    const uint32_t n = (uint32_t)get_le(head + 20, 4);
    const uint64_t wh = get_le(head + 24, 8), fh = get_le(head + 32, 8);
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return refuse("bad width or height in the header");
    if (n == 0) return refuse("a state of 0 samples");
    if (std::fseek(f, 0, SEEK_END) != 0) return refuse("cannot seek");
    const long end = std::ftell(f);
    const uint64_t want_len = kChainHeaderBytes + 16ull * w * h;
    if (end < 0) return refuse("cannot tell its length");
    if ((uint64_t)end < want_len)
        return refuse("truncated: its length is " + std::to_string(end) + " bytes, its header's " + std::to_string(w) +
                      "x" + std::to_string(h) + " needs " + std::to_string(want_len));
    if ((uint64_t)end != want_len)
        return refuse("its header's " + std::to_string(w) + "x" + std::to_string(h) + " does not match its length (" +
                      std::to_string(end) + " bytes, expected " + std::to_string(want_len) + ")");
    if (w != expect.width || h != expect.height)
        return refuse("size mismatch: the file is " + std::to_string(w) + "x" + std::to_string(h) + ", the frame " +
                      std::to_string(expect.width) + "x" + std::to_string(expect.height));
    if (wh != expect.world_hash)
        return refuse("world mismatch: the file's world hash " + hex64(wh) + ", this world's " +
                      hex64(expect.world_hash));
    if (fh != expect.frame_hash)
        return refuse("frame mismatch: the file's frame hash " + hex64(fh) + ", this frame's " +
                      hex64(expect.frame_hash));
    if (std::fseek(f, (long)kChainHeaderBytes, SEEK_SET) != 0) return refuse("cannot seek");
    std::vector<unsigned char> raw(16 * (size_t)w * h);
    if (std::fread(raw.data(), 1, raw.size(), f) != raw.size()) return refuse("truncated payload");
    state.resize(4 * (size_t)w * h);
    for (size_t i = 0; i < state.size(); ++i) state[i] = get_f32(&raw[4 * i]);
    samples = n;
    std::fclose(f);
    return true;
}

}  // namespace rtx
