// rtx_app.hpp — C++ host surface mirroring the reference's app plug-in
// interface, driven through the rtx C-ABI instead of D3D11.
//
//   RtxBase   ~ CDx11Base (CSVersion/Dx11Base.h:11-40): Initialize /
//               Terminate + pure virtual LoadContent / UnloadContent /
//               Update / Render.
//   RtxCSApp  ~ DxCSApp  (CSVersion/DxCSApp.h:12-60, DxCSApp.cpp:160-552):
//               LoadContent builds WorldDef::random_world and uploads it
//               (DxCSApp.cpp:199-418); Update computes PerFrame's camera
//               (:458-497); Render launches the path tracer (:499-552).
// Errors: bool returns like the reference (false + rtx_last_error()).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "rtx.h"

namespace rtx {

class RtxBase {
public:
    RtxBase() = default;
    virtual ~RtxBase();
    RtxBase(const RtxBase &) = delete;
    RtxBase &operator=(const RtxBase &) = delete;

    // ~ CDx11Base::Initialize(HWND, HINSTANCE) (CSVersion/Dx11Base.cpp:23-132):
    // creates the device context, then calls LoadContent.
    bool Initialize(int hip_device);
    // One frame across several devices (rtx_group, include/rtx.h): member i of
    // `devices` renders part i; all distinct devices, or all equal for the
    // one-GPU rehearsal. LoadContent / Update / Render then go through the group.
    bool Initialize(const std::vector<int> &devices, int gather_mode = RTX_GATHER_AUTO);
    // ~ CDx11Base::Terminate (CSVersion/Dx11Base.cpp:134-152).
    void Terminate();

    virtual bool LoadContent() = 0;
    virtual void UnloadContent() = 0;
    virtual void Update() = 0;
    virtual void Render() = 0;

    // The context; with a group, member 0's (the root).
    rtx_ctx *context() const { return m_ctx; }
    // The group, or null for a single context.
    rtx_group *group() const { return m_group; }
    const std::string &last_error() const { return m_error; }

protected:
    rtx_ctx *m_ctx = nullptr;      // owned, or borrowed from m_group
    rtx_group *m_group = nullptr;
    std::string m_error;
};

enum class SceneKind { RandomWorld, TestWorld, PsWorld };

struct AppConfig {
    uint32_t width = 1024, height = 576;   // texture size, DxCSApp.cpp:330-331
    uint32_t spp = 60, depth = 50;         // sceneValues, DxCSApp.cpp:133
    SceneKind scene = SceneKind::RandomWorld;
    int32_t grid_half_extent = 9;          // random_world grid, DxCSApp.cpp:95-97
    uint32_t max_spheres = 0;              // 0 = no cap
    float cam_pos[3] = {13.0f, 2.0f, 3.0f};   // DxCSApp.cpp:176
    float cam_look_at[3] = {0.0f, 0.0f, 0.0f};
    float up[3] = {0.0f, 1.0f, 0.0f};
    float vfov = 20.0f;                    // perspectiveVals, DxCSApp.cpp:179
    float aspect = 16.0f / 9.0f;
    float aperture = 2.0f;
    bool simple_camera = false;            // Camera.h instead of ComputeViewVals
    float lens_aperture = 0.0f;            // > 0: thin lens (extension, §8f-3); 0 = reference pinhole
    float focus_dist = 0.0f;               // > 0: the focus plane's distance; 0 = |cam_pos - cam_look_at| (reference)
    uint32_t rng_mode = RTX_RNG_CHAIN;
    bool lambert_guard = false;            // RTX_FRAME_LAMBERT_GUARD (extension, §8f-4); false = reference
    // Drive the library through the reference's own cbuffer bytes: LoadContent
    // fills a WorldDef (random_world, at most 512 spheres) and hands it to
    // rtx_world_from_worlddef; Update fills a PerFrame and hands it to
    // rtx_frame_from_perframe — DxCSApp's data path byte for byte.
    bool cbuffers = false;
    // With a group (RtxBase::Initialize(devices)): rows per interleaved tile.
    uint32_t tile_rows = 5;
};

// The reference's constant-buffer byte layouts (HLSL packing: float4 rows).
// WorldDef, DxCSApp.cpp:64-71: sceneValues {count, depth, spp, -1};
// spheres[512] (centre, radius); matTypes[128], four codes per float4
// (SetFloat4Cmpt, :11-17); matValues[512].
struct WorldDefBytes {
    float scene_values[4];
    float spheres[512][4];
    float mat_types[128][4];
    float mat_values[512][4];
};
static_assert(sizeof(WorldDefBytes) == 18448, "WorldDef is 18,448 bytes");
// PerFrame, DxCSApp.cpp:30-37: time, perspectiveVals {vfov, aspect,
// aperture, width}, currSamples, viewVals (4x4, stored transposed, :60).
struct PerFrameBytes {
    float time[4];
    float perspective_vals[4];
    float curr_samples[4];
    float view_vals[16];
};
static_assert(sizeof(PerFrameBytes) == 112, "PerFrame is 112 bytes");
// WorldDef::random_world into the cbuffer layout (DxCSApp.cpp:72-134); false
// if the scene does not fit its 512 slots.
bool fill_worlddef(const AppConfig &cfg, WorldDefBytes &out);
// DxCSApp::Update's PerFrame (DxCSApp.cpp:481-492): perspectiveVals,
// ComputeViewVals with focus_dist = |camPos - camLookAt|, currSamples.
bool fill_perframe(const AppConfig &cfg, float sample_count, PerFrameBytes &out);

class RtxCSApp : public RtxBase {
public:
    explicit RtxCSApp(const AppConfig &cfg = AppConfig());
    ~RtxCSApp() override;

    bool LoadContent() override;
    void UnloadContent() override;
    void Update() override;
    void Render() override;
    // Progressive frames (the reference's intended interactive mode) instead of
    // Render: `frames` more frames into the accumulator, the image rewritten.
    // With a group the frames are dealt to its members
    // (rtx_group_accumulate); otherwise `frames` calls of rtx_accumulate.
    bool Accumulate(uint32_t frames, bool reset);
    // The reference's sampleCount loop (DxCSApp.cpp:491-492) as it was meant:
    // `samples` more samples of every pixel along its own RNG chain
    // (rtx_refine), the image then the plain render's at the samples refined
    // so far. With a group every member refines its own rows
    // (rtx_group_refine, AppConfig::tile_rows) and the image is the same.
    bool Refine(uint32_t samples, bool reset);
    // Samples refined so far (rtx_refined_samples, or the group's).
    uint32_t RefinedSamples() const;
    // `samples` more samples of the pixels that are still noisy
    // (rtx_refine_adaptive: an error estimate >= threshold in the pixel's
    // 3 x 3 neighbourhood, and its count within max_samples; 0: no cap);
    // *active (may be NULL): how many were traced. With a group every member
    // refines the noisy pixels of its own rows after the members exchanged
    // their tiles' edge rows of the error map (rtx_group_refine_adaptive,
    // AppConfig::tile_rows): the image and the counts are the same.
    bool RefineAdaptive(uint32_t samples, float threshold, uint32_t max_samples, bool reset, uint32_t *active);
    // What orders a scheduled Refine's pixel queue: RTX_REFINE_KEYS_PREPASS (a
    // cost pre-pass per step, the default) or RTX_REFINE_KEYS_CARRIED (the
    // previous step's measured per-pixel cost; rtx_refine_set_keys). The
    // images are the same. With a group: every member.
    bool SetRefineKeys(int mode);
    // What every pixel shows (rtx_features): the first hit of its centre ray as
    // two planes of width * height float4, row 0 = bottom: geom = (normal,
    // depth), surf = (albedo, sphere index); a miss is (0, 0, 0, +inf) and
    // (0, 0, 0, -1). With a group: member 0, which holds the same world and frame.
    bool Features(std::vector<float> &geom, std::vector<float> &surf);
    // What is under pixel (x, y), y from the bottom row (rtx_pick). True also
    // for a miss (out->hit == 0); false when the call itself failed.
    bool Pick(uint32_t x, uint32_t y, rtx_hit *out);
    // What rays of the caller's choosing hit (rtx_cast_rays): one record per
    // ray, each over (t_min, its own t_max), through device buffers of the
    // call's own; synchronous. order: RTX_CAST_ORDER_AUTO, _GIVEN or _COHERENT,
    // a schedule and never a different record. Needs a world and no frame.
    // With a group: member 0, which holds the same world.
    bool Cast(const std::vector<rtx_ray> &rays, std::vector<rtx_ray_hit> *hits, int order = RTX_CAST_ORDER_AUTO,
              float t_min = 0.001f);
    // RTX_CAST_ORDER_GIVEN or _COHERENT: what the last Cast ran (rtx_cast_last_order).
    int CastLastOrder() const;
    // What rays of the caller's choosing see (rtx_trace_paths): `samples`
    // path-traced samples per query along the RNG chain from its seed, to the
    // world's depth; one record per query (the linear sample sum and the seed
    // after the last sample), through device buffers of the call's own;
    // synchronous. flags: RTX_PATHS_LAMBERT_GUARD, RTX_PATHS_CONTINUE — then
    // *results holds, on entry, the records to continue from, one per query.
    // segments (may be NULL): the hit_world calls this call spent per query.
    // Needs a world and no frame. With a group: member 0.
    bool TracePaths(const std::vector<rtx_path_query> &queries, uint32_t samples,
                    std::vector<rtx_path_result> *results, uint32_t flags = 0, int order = RTX_CAST_ORDER_AUTO,
                    std::vector<uint32_t> *segments = nullptr);
    // TracePaths in cost order, the longest queries first
    // (rtx_trace_paths_keyed): the records are TracePaths(..., RTX_CAST_ORDER_GIVEN)'s,
    // bit for bit. keys: NULL — the library probes with `probe` samples (0: its
    // default) — or one uint32 per query, larger for longer (probe must be 0).
    bool TracePathsKeyed(const std::vector<rtx_path_query> &queries, uint32_t samples,
                         std::vector<rtx_path_result> *results, uint32_t flags = 0,
                         const std::vector<uint32_t> *keys = nullptr, uint32_t probe = 0,
                         std::vector<uint32_t> *segments = nullptr);
    // RTX_CAST_ORDER_GIVEN or _COHERENT: what the last TracePaths ran; RTX_PATHS_ORDER_COST
    // after a TracePathsKeyed that sorted (rtx_paths_last_order).
    int PathsLastOrder() const;
    // Film queries (rtx_trace_film): `n` records at `queries` — rtx_film_query,
    // or with RTX_FILM_LENS in `flags` rtx_film_lens_query — each a pixel (fx,
    // fy) of the frame it states, `samples` jittered samples each, img_w and
    // img_h the call's (2, 2 for the unit-form records of rtx_film_camera).
    // results, flags (RTX_PATHS_*), segments: as in TracePaths. order:
    // RTX_CAST_ORDER_AUTO, _GIVEN or RTX_PATHS_ORDER_COST. Synchronous.
    bool TraceFilm(const void *queries, size_t n, uint32_t samples, float img_w, float img_h,
                   std::vector<rtx_path_result> *results, uint32_t flags = 0, int order = RTX_CAST_ORDER_AUTO,
                   std::vector<uint32_t> *segments = nullptr);
    // RTX_CAST_ORDER_GIVEN or RTX_PATHS_ORDER_COST: what the last TraceFilm ran (rtx_film_last_order).
    int FilmLastOrder() const;
    // The image of a film batch: rgba[4 * i ..] = toGamma(results[i].sum /
    // samples), alpha 1 (rtx_fold_frames on a zeroed accumulator).
    bool FilmImage(const std::vector<rtx_path_result> &results, uint32_t samples, std::vector<float> *rgba);
    // Click to focus: picks the pixel, takes the hit's plane depth
    // dot(p - cam_pos, normalize(cam_look_at - cam_pos)) as the focus distance,
    // rebuilds the frame through rtx_camera_look_at with it and sets the thin
    // lens (rtx_camera_set_aperture); later Update calls keep both
    // (AppConfig::focus_dist, lens_aperture). False on a miss (last_error()
    // says so; nothing changes) and for the simple camera and the cbuffer path.
    // A frame of other bytes ends a chain state: refine again afterwards.
    bool FocusAt(uint32_t x, uint32_t y, float aperture);
    float focus_dist() const { return m_cfg.focus_dist; }
    // "Refine that": `samples` more samples of the pixels within Chebyshev
    // distance `grow` (0..8) of one that shows a sphere of `ids` (1..256 scene
    // indices), whose count stays within max_samples (0: no cap) — the feature
    // planes, rtx_mask_from_ids and rtx_refine_masked. Needs a chain state
    // (Refine, RefineAdaptive or LoadState first). *active (may be NULL): the
    // pixels traced; *mask_pixels (may be NULL): the pixels the mask covers.
    // Under a group it returns false and says why (whole frame on one context
    // only); the app stays usable.
    bool RefineMasked(uint32_t samples, const std::vector<uint32_t> &ids, uint32_t grow, uint32_t max_samples,
                      uint32_t *active, uint32_t *mask_pixels = nullptr);
    // The chain state as a file (write_chain_state below), tagged with this
    // app's world and frame; LoadState refuses a file of another size, world
    // or frame (last_error() says which) and otherwise imports it
    // (rtx_refine_import): the image is there before anything is traced.
    // With a group the file is the same one whole-frame state
    // (rtx_group_refine_export / _import): a file saved by one context loads
    // into a group of any size and tile_rows, and the other way round.
    bool SaveState(const std::string &path);
    bool LoadState(const std::string &path);

    // Image output contract (§8f-1): the framebuffer, row 0 = image bottom.
    bool Download(std::vector<float> &rgba);
    const AppConfig &config() const { return m_cfg; }
    const rtx_frame &frame() const { return m_frame; }
    uint32_t sphere_count() const { return m_count; }
    bool ok() const { return m_ok; }

private:
    AppConfig m_cfg;
    std::vector<float> m_spheres, m_mat_types, m_mat_values;
    uint32_t m_count = 0;
    rtx_frame m_frame{};
    uint32_t m_frame_count = 0;  // ~ sampleCount, DxCSApp.cpp:491
    bool m_ok = true;
    uint32_t m_depth = 0;  // the uploaded world's depth (its hash in a chain-state file)
};

// PFM (float RGB, rows stored bottom-to-top = our row order) and binary
// PPM (8-bit, top-to-bottom: rows flipped, values clamped to [0,1]).
bool write_pfm(const std::string &path, const float *rgba, uint32_t w, uint32_t h);
bool write_ppm(const std::string &path, const float *rgba, uint32_t w, uint32_t h);

// Chain-state file (rtx_refine_export / rtx_refine_import): little-endian,
//   char[8] magic "RTXCHAIN", u32 version (1), u32 width, u32 height,
//   u32 samples (N), u64 world hash, u64 frame hash,
//   then width*height float4 (linear sum xyz, seed w), framebuffer order.
// The hashes are 64-bit FNV-1a: of the world's count, depth and its three
// arrays (spp is not part of it: refine ignores it), and of the rtx_frame bytes.
struct ChainStateHeader {
    uint32_t width = 0, height = 0, samples = 0;
    uint64_t world_hash = 0, frame_hash = 0;
};
constexpr uint32_t kChainStateVersion = 1;
uint64_t chain_world_hash(uint32_t count, uint32_t depth, const float *spheres, const float *mat_types,
                          const float *mat_values);
uint64_t chain_frame_hash(const rtx_frame &frame);
bool write_chain_state(const std::string &path, const ChainStateHeader &hdr, const float *state);
// Reads a state written for `expect`'s size, world and frame (its samples are
// ignored); `samples` receives the file's N. Refuses, with a message in `error`:
// a file that cannot be opened, a wrong magic, a wrong version, a size that
// does not match the file's length, a truncated file, and a size or hash that
// differs from `expect`.
bool read_chain_state(const std::string &path, const ChainStateHeader &expect, std::vector<float> &state,
                      uint32_t &samples, std::string &error);

}  // namespace rtx
