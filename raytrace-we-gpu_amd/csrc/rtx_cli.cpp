// rtx_cli — headless driver replacing the reference's Win32 shell
// (CSVersion/main.cpp:16-58: Initialize, one Update + Render, Terminate).
// Renders K frames, prints one JSON line of timing/counters, optionally
// writes the last frame as PFM / PPM.
//
//   rtx_cli [--width W] [--height H] [--spp S] [--depth D]
//           [--scene rtiow9|rtiow11|test|ps|random:EXT[:MAX]] [--simple-camera]
//           [--rng chain|per-sample] [--frames K] [--device N]
//           [--aperture A] [--accumulate] [--lambert-guard]
//           [--reference-frame] [--pfm out.pfm] [--ppm out.ppm]
//           [--gpus N | --devices a,b,c] [--gather auto|rccl|copy] [--tile-rows T]
//           [--split rows|frames]
//           [--refine S1,S2,...] [--save-state FILE] [--load-state FILE]
//           [--refine-keys prepass|carried]
//           [--refine-adaptive S,THRESHOLD[,MAX] --steps K] [--dump-counts FILE]
//           [--aov PREFIX] [--pick X,Y] [--focus-at X,Y] [--refine-ids S,ID[,ID...] --grow G --steps K]
//           [--cast RAYS.bin --hits OUT.bin [--cast-order auto|given|coherent] [--t-min T]]
//           [--paths QUERIES.bin --samples S [--continue] --results OUT.bin [--segments SEG.bin]
//            [--paths-order cost [--paths-probe P]] [--paths-keys KEYS.bin]]
// --paths QUERIES.bin traces the file's path queries in the scene
// (rtx_trace_paths) instead of rendering: QUERIES.bin is raw little-endian
// rtx_path_query records (32 bytes: o, seed, d, tag), OUT.bin receives one
// rtx_path_result (16 bytes: the linear sum of --samples S samples, the chain's
// seed after them) per query in the same order, SEG.bin one uint32 per query
// (the hit_world calls spent). --continue reads OUT.bin first and continues
// every query from its record. The depth is --depth's, the schedule
// --cast-order's, --lambert-guard sets RTX_PATHS_LAMBERT_GUARD. The JSON line is
// {"paths": {"queries", "samples", "segments", "order", "continued", "ms"}}.
//           [--film QUERIES.bin --film-dim W,H [--film-lens] [--film-order given|cost] --samples S
//            --results OUT.bin [--segments SEG.bin] [--continue]]
//           [--film-camera equirect|fisheye [--film-fov D] --samples S --out IMAGE.pfm|IMAGE.ppm]
// --film QUERIES.bin traces the file's film queries (rtx_trace_film) instead of
// rendering: raw 64-byte rtx_film_query records, or with --film-lens 96-byte
// rtx_film_lens_query records; --film-dim W,H are the call's img_w, img_h (2,2
// for unit-form records); --samples, --results, --segments and --continue as
// with --paths. stdout is one JSON line: {"film": {"queries", "samples",
// "segments", "order", "continued", "lens", "ms"}}. --film-camera renders the
// scene through rtx_film_camera's records of --width x --height pixels from
// the configured camera position (--film-fov: the fisheye's angle, default
// 180) and writes toGamma(sum / samples) to --out, a .pfm or a .ppm.
// --paths-order cost traces them in cost order instead (rtx_trace_paths_keyed;
// the same records, "order" says "cost" when the call sorted): by the library's
// probe of --paths-probe P samples (default 0: its own choice), or with
// --paths-keys KEYS.bin by the file's keys, one raw uint32 per query, larger
// for longer (--paths-keys alone implies --paths-order cost).
// --cast RAYS.bin casts the file's rays into the scene (rtx_cast_rays) instead
// of rendering: RAYS.bin is raw little-endian rtx_ray records (32 bytes: o,
// t_max, d, tag), OUT.bin receives one rtx_ray_hit record (32 bytes) per ray
// in the same order. --cast-order picks the schedule (default auto; the records
// do not depend on it), --t-min the rays' common t_min (default 0.001). The
// JSON line is {"cast": {"rays", "hits", "order", "t_min", "ms"}}: how many
// rays hit something, the order the call ran, and the call's wall time.
// --aov PREFIX writes the first-hit feature buffers of the frame
// (rtx_features) as PREFIX_normal.pfm, PREFIX_depth.pfm, PREFIX_albedo.pfm and
// PREFIX_id.pfm (scalars in all three channels; row 0 is the bottom, as --pfm;
// a miss has depth +inf and id -1). --pick X,Y (Y from the bottom row) adds a
// "pick" object — what rtx_pick reports for the pixel — to the JSON line.
// --focus-at X,Y, with --aperture A, puts the thin lens's focus plane on what
// that pixel shows before anything is rendered (RtxCSApp::FocusAt) and exits
// nonzero when the pixel shows nothing; the JSON line carries "focus_dist".
// --refine-ids S,ID[,ID...] with --grow G (0..8, default 0) and --steps K runs K
// masked steps of S samples (rtx_refine_masked) over the pixels that show the
// spheres ID... (grown by G pixels), after the --refine steps or the
// --load-state of the same run: it needs one of them, on one context. The
// first output line is then {"refine_masked": ...} with each step's active
// count; --dump-counts works after it.
// --refine S1,S2,... refines the image along the reference's own RNG chain,
// one rtx_refine per entry (--spp and --frames are not used): after the last
// step the image is the plain render's at spp = S1 + S2 + ... (plus a loaded
// state's samples), and --pfm / --ppm write it. --save-state FILE writes the
// chain state after the last step; --load-state FILE imports one before the
// first step (a later session continues where an earlier one stopped) and
// exits nonzero if the file is damaged or belongs to another size, world or
// frame. The JSON line then carries "refine" (the steps),
// "refined_samples" and "loaded_samples". --refine-keys carried orders each
// step's pixel queue by the previous step's measured per-pixel cost instead of
// a pre-pass per step (rtx_refine_set_keys; the image is the same), and the
// JSON line carries "refine_keys".
// --refine-adaptive S,THRESHOLD[,MAX] --steps K refines only the pixels that
// are still noisy (rtx_refine_adaptive: S samples per step, MAX the per-pixel
// cap, 0 or absent: none), until nothing is active or K steps have run, and
// prints each step's active count on stderr; the JSON line carries "active"
// (per step) and "steps_run". --dump-counts FILE writes the per-pixel sample
// counts as a PFM (the count in all three channels). --save-state works while
// the counts are uniform; a checkpoint of a non-uniform state is refused
// (RtxCSApp::SaveState).
// With --gpus / --devices, --refine refines across the group (rtx_group_refine:
// every member its own rows, tiles of --tile-rows), --save-state / --load-state
// write and read the same one whole-frame state file (a file saved by one
// context loads into a group of any size and the other way round),
// --refine-keys applies to every member, and the JSON line carries the group
// fields and the refine fields. --refine-adaptive runs on one context only.
// --gpus N renders each frame across devices 0..N-1 (rtx_group: interleaved
// tiles of T rows, default 5, one gather to device 0); --devices names them,
// and a repeated device (0,0,0) rehearses the same split on one GPU, its
// members one after another. The JSON line then also carries n_gpus, devices,
// gather, rccl_version, per_member (rows, render_ms of the last frame),
// gather_ms and deinterleave_ms, and its counters are summed over the members.
// --split frames (with --gpus / --devices; the default is rows, the above)
// renders the K frames progressively instead, whole frames dealt to the
// members in one rtx_group_accumulate(K, reset) after the warm-up (a frame, then
// one round of whole frames so that every member's buffers fit): the
// image is that of --accumulate --frames K on one context. The JSON line then
// carries "split": "frames", accumulated_frames, per_member (frames rendered,
// render_ms of the last round), gather_ms and fold_ms of the last round.
// --accumulate renders the K frames progressively (rtx_accumulate) instead
// of K independent frames, on one context (with a group: --split frames);
// --aperture enables the thin lens;
// --lambert-guard the near-zero diffuse guard (RTX_FRAME_LAMBERT_GUARD).
// --reference-frame: the reference's frame as shipped — 1024x576, spp 60,
// depth 50, random_world with 326 spheres, camera (13,2,3) -> 0, vfov 20,
// aspect 16/9 (DxCSApp.cpp:133,176-179,330-331) — uploaded as the reference's
// own WorldDef and PerFrame cbuffer bytes through rtx_world_from_worlddef /
// rtx_frame_from_perframe; a preset: every other option, before or after
// it, overrides its values.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtx_app.hpp"

static void usage() {
    std::fprintf(stderr,
                 "usage: rtx_cli [--width W] [--height H] [--spp S] [--depth D]\n"
                 "               [--scene rtiow9|rtiow11|test|ps|random:EXT[:MAX]] [--simple-camera]\n"
                 "               [--rng chain|per-sample] [--frames K] [--device N]\n"
                 "               [--aperture A] [--accumulate] [--lambert-guard] [--reference-frame]\n"
                 "               [--pfm FILE] [--ppm FILE]\n"
                 "               [--gpus N | --devices a,b,c] [--gather auto|rccl|copy] [--tile-rows T]\n"
                 "               [--split rows|frames]\n"
                 "               [--refine S1,S2,...] [--save-state FILE] [--load-state FILE]\n"
                 "               [--refine-keys prepass|carried]\n"
                 "               [--refine-adaptive S,THRESHOLD[,MAX] --steps K] [--dump-counts FILE]\n"
                 "               [--aov PREFIX] [--pick X,Y] [--focus-at X,Y]\n"
                 "               [--refine-ids S,ID[,ID...] --grow G --steps K]\n"
                 "               [--cast RAYS.bin --hits OUT.bin [--cast-order auto|given|coherent] [--t-min T]]\n"
                 "               [--paths QUERIES.bin --samples S [--continue] --results OUT.bin [--segments SEG.bin]\n"
                 "                [--paths-order cost [--paths-probe P]] [--paths-keys KEYS.bin]]\n"
                 "               [--film QUERIES.bin --film-dim W,H [--film-lens] [--film-order given|cost] --samples S\n"
                 "                --results OUT.bin [--segments SEG.bin] [--continue]]\n"
                 "               [--film-camera equirect|fisheye [--film-fov D] --samples S --out IMAGE.pfm|IMAGE.ppm]\n");
}

int main(int argc, char **argv) {
    rtx::AppConfig cfg;
    cfg.width = 1920;
    cfg.height = 1080;
    cfg.spp = 100;
    cfg.depth = 50;
    cfg.grid_half_extent = 11;
    // --reference-frame is a preset: it sets the reference's values first,
    // wherever it stands, and every other option then overrides them
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "--reference-frame") {
            cfg = rtx::AppConfig();  // the reference's values (include/rtx_app.hpp)
            cfg.cbuffers = true;
        }
    }
    int frames = 1, device = 0;
    bool accumulate = false;
    std::string pfm, ppm, save_state, load_state;
    std::vector<uint32_t> refine;  // --refine: samples per step
    int refine_keys = -1;          // --refine-keys (RTX_REFINE_KEYS_*; -1: not given)
    uint32_t ad_samples = 0, ad_max = 0;  // --refine-adaptive S,THRESHOLD[,MAX] (S 0: not given)
    float ad_threshold = 0.0f;
    int ad_steps = 1;              // --steps
    std::string dump_counts;       // --dump-counts
    std::string aov;               // --aov PREFIX
    int pick_xy[2] = {-1, -1}, focus_xy[2] = {-1, -1};  // --pick / --focus-at X,Y (-1: not given)
    uint32_t mask_samples = 0, mask_grow = 0;  // --refine-ids S,ID[,ID...] (S 0: not given), --grow
    std::vector<uint32_t> mask_ids;
    std::string cast_in, cast_out;             // --cast RAYS.bin, --hits OUT.bin
    int cast_order = RTX_CAST_ORDER_AUTO;      // --cast-order
    float cast_t_min = 0.001f;                 // --t-min
    std::string paths_in, paths_out, paths_seg;  // --paths QUERIES.bin, --results OUT.bin, --segments SEG.bin
    long paths_samples = 0;                    // --samples
    bool paths_continue = false;               // --continue
    bool paths_cost = false;                   // --paths-order cost
    long paths_probe = 0;                      // --paths-probe
    std::string paths_keys;                    // --paths-keys KEYS.bin
    std::string film_in, film_out;             // --film QUERIES.bin, --out IMAGE
    float film_dim[2] = {0.0f, 0.0f};          // --film-dim W,H
    bool film_lens = false, film_dim_set = false;  // --film-lens
    int film_order = RTX_CAST_ORDER_GIVEN;     // --film-order
    int film_camera = -1;                      // --film-camera (RTX_FILM_*; -1: not given)
    float film_fov = 180.0f;                   // --film-fov
    std::vector<int> devices;  // non-empty: a group
    int gather = RTX_GATHER_AUTO;
    bool group_opts = false;   // --gather / --tile-rows given
    bool split_frames = false; // --split frames: progressive frames dealt to the members
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) {
                usage();
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--width") cfg.width = (uint32_t)std::atoi(next());
        else if (a == "--height") cfg.height = (uint32_t)std::atoi(next());
        else if (a == "--spp") cfg.spp = (uint32_t)std::atoi(next());
        else if (a == "--depth") cfg.depth = (uint32_t)std::atoi(next());
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--pfm") pfm = next();
        else if (a == "--ppm") ppm = next();
        else if (a == "--save-state") save_state = next();
        else if (a == "--load-state") load_state = next();
        else if (a == "--refine") {
            refine.clear();
            const std::string list = next();
            for (size_t pos = 0; pos <= list.size();) {
                const size_t comma = std::min(list.find(',', pos), list.size());
                const std::string item = list.substr(pos, comma - pos);
                const unsigned long long v = item.empty() || item.size() > 10 ||
                                                     item.find_first_not_of("0123456789") != std::string::npos
                                                 ? 0ull
                                                 : std::strtoull(item.c_str(), nullptr, 10);
                if (v == 0ull || v > 0xffffffffull) {
                    usage();
                    return 2;
                }
                refine.push_back((uint32_t)v);
                pos = comma + 1;
            }
        }
        else if (a == "--refine-adaptive") {
            unsigned long long s = 0, m = 0;
            float t = 0.0f;
            char tail = 0;
            const int got = std::sscanf(next(), "%llu,%f,%llu%c", &s, &t, &m, &tail);
            if ((got != 2 && got != 3) || s == 0ull || s > 0xffffffffull || m > 0xffffffffull || t != t) {
                usage();
                return 2;
            }
            ad_samples = (uint32_t)s;
            ad_threshold = t;
            ad_max = (uint32_t)m;
        }
        else if (a == "--steps") ad_steps = std::atoi(next());
        else if (a == "--aov") aov = next();
        else if (a == "--pick" || a == "--focus-at") {
            int *xy = a == "--pick" ? pick_xy : focus_xy;
            char tail = 0;
            if (std::sscanf(next(), "%d,%d%c", &xy[0], &xy[1], &tail) != 2 || xy[0] < 0 || xy[1] < 0) {
                usage();
                return 2;
            }
        }
        else if (a == "--grow") mask_grow = (uint32_t)std::atoi(next());
        else if (a == "--refine-ids") {
            std::vector<uint32_t> v;
            const std::string list = next();
            for (size_t pos = 0; pos <= list.size();) {
                const size_t comma = std::min(list.find(',', pos), list.size());
                const std::string item = list.substr(pos, comma - pos);
                if (item.empty() || item.size() > 9 || item.find_first_not_of("0123456789") != std::string::npos) {
                    usage();
                    return 2;
                }
                v.push_back((uint32_t)std::strtoul(item.c_str(), nullptr, 10));
                pos = comma + 1;
            }
            if (v.size() < 2 || v[0] == 0u) {
                usage();
                return 2;
            }
            mask_samples = v[0];
            mask_ids.assign(v.begin() + 1, v.end());
        }
        else if (a == "--dump-counts") dump_counts = next();
        else if (a == "--cast") cast_in = next();
        else if (a == "--hits") cast_out = next();
        else if (a == "--paths") paths_in = next();
        else if (a == "--results") paths_out = next();
        else if (a == "--segments") paths_seg = next();
        else if (a == "--samples") paths_samples = std::atol(next());
        else if (a == "--continue") paths_continue = true;
        else if (a == "--paths-order") {
            if (std::string(next()) != "cost") usage();
            paths_cost = true;
        } else if (a == "--paths-probe") paths_probe = std::atol(next());
        else if (a == "--paths-keys") paths_keys = next(), paths_cost = true;
        else if (a == "--film") film_in = next();
        else if (a == "--out") film_out = next();
        else if (a == "--film-lens") film_lens = true;
        else if (a == "--film-fov") film_fov = (float)std::atof(next());
        else if (a == "--film-dim") {
            char tail = 0;
            if (std::sscanf(next(), "%f,%f%c", &film_dim[0], &film_dim[1], &tail) != 2) {
                usage();
                return 2;
            }
            film_dim_set = true;
        } else if (a == "--film-order") {
            const std::string m = next();
            if (m == "given") film_order = RTX_CAST_ORDER_GIVEN;
            else if (m == "cost") film_order = RTX_PATHS_ORDER_COST;
            else {
                usage();
                return 2;
            }
        } else if (a == "--film-camera") {
            const std::string m = next();
            if (m == "equirect") film_camera = RTX_FILM_EQUIRECT;
            else if (m == "fisheye") film_camera = RTX_FILM_FISHEYE;
            else {
                usage();
                return 2;
            }
        }
        else if (a == "--t-min") cast_t_min = (float)std::atof(next());
        else if (a == "--cast-order") {
            const std::string m = next();
            if (m == "auto") cast_order = RTX_CAST_ORDER_AUTO;
            else if (m == "given") cast_order = RTX_CAST_ORDER_GIVEN;
            else if (m == "coherent") cast_order = RTX_CAST_ORDER_COHERENT;
            else {
                usage();
                return 2;
            }
        }
        else if (a == "--refine-keys") {
            const std::string m = next();
            if (m == "prepass") refine_keys = RTX_REFINE_KEYS_PREPASS;
            else if (m == "carried") refine_keys = RTX_REFINE_KEYS_CARRIED;
            else {
                usage();
                return 2;
            }
        }
        else if (a == "--simple-camera") cfg.simple_camera = true;
        else if (a == "--aperture") cfg.lens_aperture = (float)std::atof(next());
        else if (a == "--accumulate") accumulate = true;
        else if (a == "--lambert-guard") cfg.lambert_guard = true;
        else if (a == "--gpus") {
            const int n = std::atoi(next());
            if (n < 1 || n > RTX_GROUP_MAX) {
                usage();
                return 2;
            }
            devices.clear();
            for (int d = 0; d < n; ++d) devices.push_back(d);
        } else if (a == "--devices") {
            devices.clear();
            const std::string list = next();
            for (size_t pos = 0; pos <= list.size();) {
                const size_t comma = std::min(list.find(',', pos), list.size());
                const std::string item = list.substr(pos, comma - pos);
                if (item.empty() || item.find_first_not_of("0123456789") != std::string::npos) {
                    usage();
                    return 2;
                }
                devices.push_back(std::atoi(item.c_str()));
                pos = comma + 1;
            }
        } else if (a == "--gather") {
            const std::string m = next();
            group_opts = true;
            if (m == "auto") gather = RTX_GATHER_AUTO;
            else if (m == "rccl") gather = RTX_GATHER_RCCL;
            else if (m == "copy") gather = RTX_GATHER_COPY;
            else {
                usage();
                return 2;
            }
        } else if (a == "--split") {
            const std::string m = next();
            if (m == "frames") split_frames = true;
            else if (m == "rows") split_frames = false;
            else {
                usage();
                return 2;
            }
        } else if (a == "--tile-rows") {
            cfg.tile_rows = (uint32_t)std::atoi(next());
            group_opts = true;
        }
        else if (a == "--reference-frame") {
            // a preset, applied before the loop (below): here it only keeps its place
        }
        else if (a == "--rng") {
            const std::string m = next();
            cfg.rng_mode = (m == "per-sample") ? RTX_RNG_PER_SAMPLE : RTX_RNG_CHAIN;
        } else if (a == "--scene") {
            const std::string s = next();
            if (s == "rtiow9") cfg.grid_half_extent = 9;
            else if (s == "rtiow11") cfg.grid_half_extent = 11;
            else if (s == "test") cfg.scene = rtx::SceneKind::TestWorld;
            else if (s == "ps") cfg.scene = rtx::SceneKind::PsWorld;
            else if (s.rfind("random:", 0) == 0) {
                unsigned ext = 0, mx = 0;
                if (std::sscanf(s.c_str() + 7, "%u:%u", &ext, &mx) < 1) {
                    usage();
                    return 2;
                }
                cfg.grid_half_extent = (int32_t)ext;
                cfg.max_spheres = mx;
            } else {
                usage();
                return 2;
            }
        } else {
            usage();
            return 2;
        }
    }
    if (cfg.width == 0 || cfg.height == 0 || frames < 1) {
        usage();
        return 2;
    }
    const bool grouped = !devices.empty();
    if (group_opts && !grouped) {
        std::fprintf(stderr, "rtx_cli: --gather and --tile-rows need --gpus or --devices\n");
        return 2;
    }
    if (split_frames && !grouped) {
        std::fprintf(stderr, "rtx_cli: --split frames needs --gpus or --devices\n");
        return 2;
    }
    if (grouped && accumulate) {
        std::fprintf(stderr, "rtx_cli: --accumulate with --gpus / --devices is not supported "
                             "(a group accumulates with --split frames)\n");
        return 2;
    }
    if (cast_in.empty() != cast_out.empty()) {
        std::fprintf(stderr, "rtx_cli: --cast RAYS.bin and --hits OUT.bin go together\n");
        return 2;
    }
    if ((paths_in.empty() && film_in.empty()) != paths_out.empty() || (!paths_in.empty() && !cast_in.empty())) {
        std::fprintf(stderr, "rtx_cli: --paths QUERIES.bin and --results OUT.bin go together, without --cast\n");
        return 2;
    }
    if (!paths_in.empty() && (paths_samples < 1 || paths_samples > 0xffffffffl)) {
        std::fprintf(stderr, "rtx_cli: --paths needs --samples S >= 1\n");
        return 2;
    }
    const bool filming = !film_in.empty() || film_camera >= 0;
    if (filming && (!paths_in.empty() || !cast_in.empty() || (!film_in.empty() && film_camera >= 0))) {
        std::fprintf(stderr, "rtx_cli: --film and --film-camera go alone, without --paths and --cast\n");
        return 2;
    }
    if (!film_in.empty() && (paths_out.empty() || !film_dim_set || !film_out.empty())) {
        std::fprintf(stderr, "rtx_cli: --film QUERIES.bin needs --film-dim W,H and --results OUT.bin (no --out)\n");
        return 2;
    }
    if (film_camera >= 0 && (film_out.size() < 5 || (film_out.substr(film_out.size() - 4) != ".pfm" &&
                                                      film_out.substr(film_out.size() - 4) != ".ppm") ||
                             !paths_out.empty() || !paths_seg.empty() || paths_continue)) {
        std::fprintf(stderr, "rtx_cli: --film-camera needs --out IMAGE.pfm or IMAGE.ppm, without --results, "
                             "--segments and --continue\n");
        return 2;
    }
    if (filming && (paths_samples < 1 || paths_samples > 0xffffffffl)) {
        std::fprintf(stderr, "rtx_cli: --film and --film-camera need --samples S >= 1\n");
        return 2;
    }
    if (!filming && (film_lens || film_dim_set || !film_out.empty())) {
        std::fprintf(stderr, "rtx_cli: --film-dim and --film-lens go with --film, --out with --film-camera\n");
        return 2;
    }
    if (paths_in.empty() && !filming && (paths_continue || !paths_seg.empty() || paths_samples != 0)) {
        std::fprintf(stderr, "rtx_cli: --samples, --continue and --segments go with --paths\n");
        return 2;
    }
    if ((paths_in.empty() && (paths_cost || paths_probe != 0)) || paths_probe < 0 || paths_probe > 0xffffffffl ||
        (paths_probe != 0 && !paths_keys.empty())) {
        std::fprintf(stderr, "rtx_cli: --paths-order, --paths-probe P >= 0 and --paths-keys go with --paths; "
                             "--paths-probe goes without --paths-keys\n");
        return 2;
    }
    const bool adaptive = ad_samples != 0u;
    if (adaptive && (!refine.empty() || !load_state.empty() || ad_steps < 1)) {
        std::fprintf(stderr, "rtx_cli: --refine-adaptive takes --steps K >= 1, without --refine and --load-state\n");
        return 2;
    }
    const bool masked = mask_samples != 0u;
    if (masked && refine.empty() && load_state.empty()) {
        std::fprintf(stderr, "rtx_cli: --refine-ids continues a chain state: it needs --refine or --load-state in the "
                             "same run\n");
        return 2;
    }
    if (masked && (adaptive || ad_steps < 1 || !devices.empty())) {
        std::fprintf(stderr, "rtx_cli: --refine-ids takes --steps K >= 1, without --refine-adaptive, on one context\n");
        return 2;
    }
    if (!dump_counts.empty() && !adaptive && !masked) {
        std::fprintf(stderr, "rtx_cli: --dump-counts needs --refine-adaptive or --refine-ids\n");
        return 2;
    }
    if (focus_xy[0] >= 0 && !(cfg.lens_aperture > 0.0f)) {
        std::fprintf(stderr, "rtx_cli: --focus-at needs --aperture A > 0\n");
        return 2;
    }
    const bool refining = !refine.empty() || adaptive || masked;
    if ((!save_state.empty() || !load_state.empty()) && !refining) {
        std::fprintf(stderr, "rtx_cli: --save-state and --load-state need --refine\n");
        return 2;
    }
    if (refine_keys >= 0 && !refining) {
        std::fprintf(stderr, "rtx_cli: --refine-keys needs --refine\n");
        return 2;
    }
    if (refining && (accumulate || split_frames)) {
        std::fprintf(stderr, "rtx_cli: --refine runs without --accumulate and --split frames\n");
        return 2;
    }
    if (adaptive && grouped) {
        std::fprintf(stderr, "rtx_cli: --refine-adaptive runs on one context (a group refines with --refine)\n");
        return 2;
    }
    if (grouped && cfg.tile_rows == 0) {
        usage();
        return 2;
    }
    cfg.aspect = (float)cfg.width / (float)cfg.height;
    rtx::RtxCSApp app(cfg);
    if (!(grouped ? app.Initialize(devices, gather) : app.Initialize(device))) {
        std::fprintf(stderr, "rtx_cli: initialize failed: %s\n", app.last_error().c_str());
        return 1;
    }
    app.Update();
    if (!cast_in.empty()) {  // cast the file's rays instead of rendering
        std::vector<rtx_ray> rays;
        std::FILE *f = std::fopen(cast_in.c_str(), "rb");
        bool ok = f != nullptr;
        if (ok) {
            ok = std::fseek(f, 0, SEEK_END) == 0;
            const long bytes = ok ? std::ftell(f) : -1;
            ok = ok && bytes >= 0 && bytes % (long)sizeof(rtx_ray) == 0 && std::fseek(f, 0, SEEK_SET) == 0;
            if (ok) {
                rays.resize((size_t)bytes / sizeof(rtx_ray));
                ok = std::fread(rays.data(), sizeof(rtx_ray), rays.size(), f) == rays.size();
            }
            std::fclose(f);
        }
        if (!ok) {
            std::fprintf(stderr, "rtx_cli: --cast: cannot read %s as 32-byte ray records\n", cast_in.c_str());
            return 1;
        }
        std::vector<rtx_ray_hit> hits;
        const auto t0 = std::chrono::steady_clock::now();
        if (!app.Cast(rays, &hits, cast_order, cast_t_min)) {
            std::fprintf(stderr, "rtx_cli: --cast failed: %s\n", app.last_error().c_str());
            return 1;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        f = std::fopen(cast_out.c_str(), "wb");
        ok = f != nullptr && std::fwrite(hits.data(), sizeof(rtx_ray_hit), hits.size(), f) == hits.size();
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "rtx_cli: --hits: cannot write %s\n", cast_out.c_str());
            return 1;
        }
        size_t nhit = 0;
        for (const rtx_ray_hit &h : hits) nhit += h.index >= 0;
        std::printf("{\"cast\": {\"rays\": %zu, \"hits\": %zu, \"order\": \"%s\", \"t_min\": %.9g, \"ms\": %.3f}}\n",
                    rays.size(), nhit, app.CastLastOrder() == RTX_CAST_ORDER_COHERENT ? "coherent" : "given",
                    (double)cast_t_min, ms);
        return 0;
    }
    if (filming) {  // trace film queries instead of rendering: the file's, or a camera model's
        std::vector<unsigned char> raw;
        const size_t rec = film_lens ? sizeof(rtx_film_lens_query) : sizeof(rtx_film_query);
        float img_w = film_dim[0], img_h = film_dim[1];
        auto read_all = [](const std::string &path, size_t unit, std::vector<unsigned char> &out) {
            std::FILE *f = std::fopen(path.c_str(), "rb");
            bool ok = f != nullptr;
            if (ok) {
                ok = std::fseek(f, 0, SEEK_END) == 0;
                const long bytes = ok ? std::ftell(f) : -1;
                ok = ok && bytes >= 0 && bytes % (long)unit == 0 && std::fseek(f, 0, SEEK_SET) == 0;
                if (ok) {
                    out.resize((size_t)bytes);
                    ok = std::fread(out.data(), 1, out.size(), f) == out.size();
                }
                std::fclose(f);
            }
            return ok;
        };
        auto write_all = [](const std::string &path, const void *data, size_t bytes) {
            std::FILE *f = std::fopen(path.c_str(), "wb");
            bool ok = f != nullptr && std::fwrite(data, 1, bytes, f) == bytes;
            if (f) ok = std::fclose(f) == 0 && ok;
            return ok;
        };
        if (film_camera >= 0) {
            const float up[3] = {0.0f, 1.0f, 0.0f};
            raw.resize((size_t)cfg.width * cfg.height * sizeof(rtx_film_query));
            if (rtx_film_camera(film_camera, cfg.cam_pos, cfg.cam_look_at, up, film_fov, cfg.width, cfg.height, 0,
                                reinterpret_cast<rtx_film_query *>(raw.data())) != RTX_OK) {
                std::fprintf(stderr, "rtx_cli: --film-camera: bad --film-fov, --width or --height\n");
                return 2;
            }
            img_w = img_h = 2.0f;  // unit-form records
        } else if (!read_all(film_in, rec, raw)) {
            std::fprintf(stderr, "rtx_cli: --film: cannot read %s as %zu-byte query records\n", film_in.c_str(), rec);
            return 1;
        }
        const size_t nq = raw.size() / rec;
        std::vector<rtx_path_result> results;
        if (paths_continue) {
            std::vector<unsigned char> prev;
            if (!read_all(paths_out, sizeof(rtx_path_result), prev) || prev.size() != nq * sizeof(rtx_path_result)) {
                std::fprintf(stderr, "rtx_cli: --continue: cannot read %s as one 16-byte record per query\n",
                             paths_out.c_str());
                return 1;
            }
            results.resize(nq);
            if (!prev.empty()) std::memcpy(results.data(), prev.data(), prev.size());
        }
        std::vector<uint32_t> segs;
        const uint32_t fflags = (paths_continue ? (uint32_t)RTX_PATHS_CONTINUE : 0u) |
                                (cfg.lambert_guard ? (uint32_t)RTX_PATHS_LAMBERT_GUARD : 0u) |
                                (film_lens ? (uint32_t)RTX_FILM_LENS : 0u);
        const auto t0 = std::chrono::steady_clock::now();
        if (!app.TraceFilm(raw.data(), nq, (uint32_t)paths_samples, img_w, img_h, &results, fflags, film_order, &segs)) {
            std::fprintf(stderr, "rtx_cli: --film failed: %s\n", app.last_error().c_str());
            return 1;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (film_camera >= 0) {
            std::vector<float> img;
            if (!app.FilmImage(results, (uint32_t)paths_samples, &img)) {
                std::fprintf(stderr, "rtx_cli: --film-camera failed: %s\n", app.last_error().c_str());
                return 1;
            }
            const bool is_pfm = film_out.substr(film_out.size() - 4) == ".pfm";
            if (!(is_pfm ? rtx::write_pfm(film_out, img.data(), cfg.width, cfg.height)
                         : rtx::write_ppm(film_out, img.data(), cfg.width, cfg.height))) {
                std::fprintf(stderr, "rtx_cli: --out: cannot write %s\n", film_out.c_str());
                return 1;
            }
        } else {
            if (!write_all(paths_out, results.data(), results.size() * sizeof(rtx_path_result))) {
                std::fprintf(stderr, "rtx_cli: --results: cannot write %s\n", paths_out.c_str());
                return 1;
            }
            if (!paths_seg.empty() && !write_all(paths_seg, segs.data(), segs.size() * sizeof(uint32_t))) {
                std::fprintf(stderr, "rtx_cli: --segments: cannot write %s\n", paths_seg.c_str());
                return 1;
            }
        }
        unsigned long long total = 0;
        for (const uint32_t v : segs) total += v;
        std::printf("{\"film\": {\"queries\": %zu, \"samples\": %ld, \"segments\": %llu, \"order\": \"%s\", "
                    "\"continued\": %s, \"lens\": %s, \"ms\": %.3f}}\n",
                    nq, paths_samples, total, app.FilmLastOrder() == RTX_PATHS_ORDER_COST ? "cost" : "given",
                    paths_continue ? "true" : "false", film_lens ? "true" : "false", ms);
        return 0;
    }
    if (!paths_in.empty()) {  // trace the file's path queries instead of rendering
        // a file of whole records; false: unreadable, or not a multiple of the record size
        auto slurp = [](const std::string &path, size_t rec, std::vector<unsigned char> &out) {
            std::FILE *f = std::fopen(path.c_str(), "rb");
            bool ok = f != nullptr;
            if (ok) {
                ok = std::fseek(f, 0, SEEK_END) == 0;
                const long bytes = ok ? std::ftell(f) : -1;
                ok = ok && bytes >= 0 && bytes % (long)rec == 0 && std::fseek(f, 0, SEEK_SET) == 0;
                if (ok) {
                    out.resize((size_t)bytes);
                    ok = std::fread(out.data(), 1, out.size(), f) == out.size();
                }
                std::fclose(f);
            }
            return ok;
        };
        auto spill = [](const std::string &path, const void *data, size_t bytes) {
            std::FILE *f = std::fopen(path.c_str(), "wb");
            bool ok = f != nullptr && std::fwrite(data, 1, bytes, f) == bytes;
            if (f) ok = std::fclose(f) == 0 && ok;
            return ok;
        };
        std::vector<unsigned char> raw;
        if (!slurp(paths_in, sizeof(rtx_path_query), raw)) {
            std::fprintf(stderr, "rtx_cli: --paths: cannot read %s as 32-byte query records\n", paths_in.c_str());
            return 1;
        }
        std::vector<rtx_path_query> queries(raw.size() / sizeof(rtx_path_query));
        if (!raw.empty()) std::memcpy(queries.data(), raw.data(), raw.size());
        std::vector<rtx_path_result> results;
        if (paths_continue) {
            if (!slurp(paths_out, sizeof(rtx_path_result), raw) ||
                raw.size() != queries.size() * sizeof(rtx_path_result)) {
                std::fprintf(stderr, "rtx_cli: --continue: cannot read %s as one 16-byte record per query\n",
                             paths_out.c_str());
                return 1;
            }
            results.resize(queries.size());
            if (!raw.empty()) std::memcpy(results.data(), raw.data(), raw.size());
        }
        std::vector<uint32_t> segs, keys;
        if (!paths_keys.empty()) {
            if (!slurp(paths_keys, sizeof(uint32_t), raw) || raw.size() != queries.size() * sizeof(uint32_t)) {
                std::fprintf(stderr, "rtx_cli: --paths-keys: cannot read %s as one uint32 per query\n",
                             paths_keys.c_str());
                return 1;
            }
            keys.resize(queries.size());
            if (!raw.empty()) std::memcpy(keys.data(), raw.data(), raw.size());
        }
        const uint32_t pflags = (paths_continue ? (uint32_t)RTX_PATHS_CONTINUE : 0u) |
                                (cfg.lambert_guard ? (uint32_t)RTX_PATHS_LAMBERT_GUARD : 0u);
        const auto t0 = std::chrono::steady_clock::now();
        if (!(paths_cost ? app.TracePathsKeyed(queries, (uint32_t)paths_samples, &results, pflags,
                                               paths_keys.empty() ? nullptr : &keys, (uint32_t)paths_probe, &segs)
                         : app.TracePaths(queries, (uint32_t)paths_samples, &results, pflags, cast_order, &segs))) {
            std::fprintf(stderr, "rtx_cli: --paths failed: %s\n", app.last_error().c_str());
            return 1;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!spill(paths_out, results.data(), results.size() * sizeof(rtx_path_result))) {
            std::fprintf(stderr, "rtx_cli: --results: cannot write %s\n", paths_out.c_str());
            return 1;
        }
        if (!paths_seg.empty() && !spill(paths_seg, segs.data(), segs.size() * sizeof(uint32_t))) {
            std::fprintf(stderr, "rtx_cli: --segments: cannot write %s\n", paths_seg.c_str());
            return 1;
        }
        unsigned long long total = 0;
        for (const uint32_t v : segs) total += v;
        std::printf("{\"paths\": {\"queries\": %zu, \"samples\": %ld, \"segments\": %llu, \"order\": \"%s\", "
                    "\"continued\": %s, \"ms\": %.3f}}\n",
                    queries.size(), paths_samples, total,
                    app.PathsLastOrder() == RTX_PATHS_ORDER_COST      ? "cost"
                    : app.PathsLastOrder() == RTX_CAST_ORDER_COHERENT ? "coherent"
                                                                      : "given",
                    paths_continue ? "true" : "false", ms);
        return 0;
    }
    std::string extra;  // further fields of the JSON line: "focus_dist", "pick"
    if (focus_xy[0] >= 0) {
        if (!app.FocusAt((uint32_t)focus_xy[0], (uint32_t)focus_xy[1], cfg.lens_aperture)) {
            std::fprintf(stderr, "rtx_cli: --focus-at failed: %s\n", app.last_error().c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof buf, ", \"focus_dist\": %.9g", (double)app.focus_dist());
        extra += buf;
    }
    if (pick_xy[0] >= 0) {
        rtx_hit h{};
        if (!app.Pick((uint32_t)pick_xy[0], (uint32_t)pick_xy[1], &h)) {
            std::fprintf(stderr, "rtx_cli: --pick failed: %s\n", app.last_error().c_str());
            return 1;
        }
        char buf[640];
        // (a miss's depth is +inf, which JSON cannot hold: null)
        char depth[32];
        if (h.hit) std::snprintf(depth, sizeof depth, "%.9g", (double)h.depth);
        else std::snprintf(depth, sizeof depth, "null");
        std::snprintf(buf, sizeof buf,
                      ", \"pick\": {\"x\": %d, \"y\": %d, \"hit\": %u, \"index\": %d, \"front_face\": %u, "
                      "\"material\": %u, \"t\": %.9g, \"depth\": %s, \"p\": [%.9g, %.9g, %.9g], "
                      "\"normal\": [%.9g, %.9g, %.9g], \"albedo\": [%.9g, %.9g, %.9g], \"mat_param\": %.9g}",
                      pick_xy[0], pick_xy[1], h.hit, h.index, h.front_face, h.material, (double)h.t, depth,
                      (double)h.p[0], (double)h.p[1], (double)h.p[2], (double)h.normal[0], (double)h.normal[1],
                      (double)h.normal[2], (double)h.albedo[0], (double)h.albedo[1], (double)h.albedo[2],
                      (double)h.mat_param);
        extra += buf;
    }
    if (!aov.empty()) {
        std::vector<float> geom, surf;
        if (!app.Features(geom, surf)) {
            std::fprintf(stderr, "rtx_cli: --aov failed: %s\n", app.last_error().c_str());
            return 1;
        }
        const size_t px = (size_t)cfg.width * cfg.height;
        std::vector<float> depth(4 * px), id(4 * px);
        for (size_t i = 0; i < px; ++i)
            for (int c = 0; c < 4; ++c) {
                depth[4 * i + c] = geom[4 * i + 3];
                id[4 * i + c] = surf[4 * i + 3];
            }
        if (!rtx::write_pfm(aov + "_normal.pfm", geom.data(), cfg.width, cfg.height) ||
            !rtx::write_pfm(aov + "_depth.pfm", depth.data(), cfg.width, cfg.height) ||
            !rtx::write_pfm(aov + "_albedo.pfm", surf.data(), cfg.width, cfg.height) ||
            !rtx::write_pfm(aov + "_id.pfm", id.data(), cfg.width, cfg.height)) {
            std::fprintf(stderr, "rtx_cli: --aov: cannot write %s_*.pfm\n", aov.c_str());
            return 1;
        }
    }
    uint32_t loaded_samples = 0;
    if (refining) {
        if (refine_keys >= 0 && !app.SetRefineKeys(refine_keys)) {
            std::fprintf(stderr, "rtx_cli: --refine-keys failed: %s\n", app.last_error().c_str());
            return 1;
        }
        // no warm-up frame: every step's samples count. A saved state first.
        if (!load_state.empty()) {
            if (!app.LoadState(load_state)) {
                std::fprintf(stderr, "rtx_cli: --load-state refused: %s\n", app.last_error().c_str());
                return 1;
            }
            loaded_samples = app.RefinedSamples();
        }
    } else {
        app.Render();  // warm-up frame (also the reference's single frame, main.cpp:38-39)
    }
    // ... and one round of whole frames: the row-split warm-up sized every member's
    // buffers for its rows only, and the timed call is to find them fitting
    if (split_frames) app.Accumulate((uint32_t)devices.size(), true);
    rtx_group *grp = app.group();
    const uint32_t members = grp ? rtx_group_size(grp) : 0;
    if (grp) {
        rtx_group_sync(grp);
        for (uint32_t m = 0; m < members; ++m) rtx_stats_reset(rtx_group_ctx(grp, m));
    } else {
        rtx_sync(app.context());
        rtx_stats_reset(app.context());
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (split_frames) {
        app.Update();
        app.Accumulate((uint32_t)frames, true);
    }
    for (size_t k = 0; k < refine.size(); ++k) {
        app.Update();  // the same PerFrame bytes every Update: the chain state is kept
        if (!app.Refine(refine[k], k == 0 && load_state.empty())) break;
    }
    std::vector<uint32_t> ad_active;  // --refine-adaptive: pixels traced per step
    for (int k = 0; adaptive && k < ad_steps; ++k) {
        app.Update();
        uint32_t n = 0;
        if (!app.RefineAdaptive(ad_samples, ad_threshold, ad_max, k == 0, &n)) break;
        std::fprintf(stderr, "rtx_cli: adaptive step %d: %u active\n", k + 1, n);
        if (n == 0u) break;  // nothing is noisy any more (or every pixel is at its cap)
        ad_active.push_back(n);
    }
    std::vector<uint32_t> mask_active;  // --refine-ids: pixels traced per step
    uint32_t mask_pixels = 0;
    for (int k = 0; masked && k < ad_steps; ++k) {
        app.Update();
        uint32_t n = 0;
        if (!app.RefineMasked(mask_samples, mask_ids, mask_grow, 0, &n, &mask_pixels)) {
            std::fprintf(stderr, "rtx_cli: --refine-ids failed: %s\n", app.last_error().c_str());
            return 1;
        }
        std::fprintf(stderr, "rtx_cli: masked step %d: %u active of %u masked\n", k + 1, n, mask_pixels);
        mask_active.push_back(n);
    }
    for (int k = 0; k < frames && !split_frames && !refining; ++k) {
        app.Update();
        if (accumulate) {
            if (rtx_accumulate(app.context(), k == 0) != RTX_OK) {
                std::fprintf(stderr, "rtx_cli: accumulate failed: %s\n", rtx_last_error());
                return 1;
            }
        } else {
            app.Render();
        }
    }
    const int sync_rc = grp ? rtx_group_sync(grp) : rtx_sync(app.context());
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!app.ok()) {
        std::fprintf(stderr, "rtx_cli: render failed: %s\n", app.last_error().c_str());
        return 1;
    }
    rtx_stats st{};
    if (grp) {
        if (sync_rc != RTX_OK) {
            std::fprintf(stderr, "rtx_cli: render failed: %s\n", rtx_last_error());
            return 1;
        }
        for (uint32_t m = 0; m < members; ++m) {  // the counters, summed over the members
            rtx_stats s{};
            if (rtx_get_stats(rtx_group_ctx(grp, m), &s) != RTX_OK) {
                std::fprintf(stderr, "rtx_cli: member %u stats failed: %s\n", m, rtx_last_error());
                return 1;
            }
            st.kernel_ms += s.kernel_ms;
            st.launches += s.launches;
            st.samples += s.samples;
            st.segments += s.segments;
            st.sphere_tests += s.sphere_tests;
        }
        std::vector<double> render_ms(members, 0.0);
        double gather_ms = 0.0, deint_ms = 0.0;  // (deint_ms: with --split frames the fold)
        if ((split_frames ? rtx_group_get_accumulate_times(grp, render_ms.data(), &gather_ms, &deint_ms)
                          : rtx_group_get_times(grp, render_ms.data(), &gather_ms, &deint_ms)) != RTX_OK) {
            std::fprintf(stderr, "rtx_cli: times failed: %s\n", rtx_last_error());
            return 1;
        }
        std::string devs, per;
        char buf[96];
        for (uint32_t m = 0; m < members; ++m) {
            devs += (m ? ", " : "") + std::to_string(devices[m]);
            if (split_frames)  // frame j goes to member j % n
                std::snprintf(buf, sizeof buf, "%s{\"frames\": %u, \"render_ms\": %.4f}", m ? ", " : "",
                              (uint32_t)frames / members + (m < (uint32_t)frames % members ? 1u : 0u), render_ms[m]);
            else
                std::snprintf(buf, sizeof buf, "%s{\"rows\": %u, \"render_ms\": %.4f}", m ? ", " : "",
                              rtx_part_rows(cfg.height, cfg.tile_rows, m, members), render_ms[m]);
            per += buf;
        }
        const int ver = rtx_group_rccl_version(grp);
        const std::string rccl = ver ? "\"" + std::to_string(ver) + "\"" : "null";
        // the row split names its tile_rows and the de-interleave, the frame split its frames and the fold
        const std::string split = split_frames ? "\"split\": \"frames\", \"accumulated_frames\": " +
                                                     std::to_string(rtx_group_accumulated_frames(grp))
                                               : "\"tile_rows\": " + std::to_string(cfg.tile_rows);
        // a refining group: the refine line's fields as well
        std::string ref;
        if (refining) {
            std::string steps;
            for (size_t k = 0; k < refine.size(); ++k) steps += (k ? ", " : "") + std::to_string(refine[k]);
            ref = ", \"refine\": [" + steps + "], \"loaded_samples\": " + std::to_string(loaded_samples) +
                  ", \"refined_samples\": " + std::to_string(app.RefinedSamples()) + ", \"refine_keys\": \"" +
                  (refine_keys == RTX_REFINE_KEYS_CARRIED ? "carried" : "prepass") + "\"";
        }
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %u, \"depth\": %u, \"spheres\": %u, "
                    "\"cbuffers\": %s, \"frames\": %d, \"wall_s\": %.6f, \"kernel_ms\": %.4f, "
                    "\"msamples_per_s\": %.3f, \"segments\": %llu, \"sphere_tests\": %llu, "
                    "\"n_gpus\": %u, \"devices\": [%s], \"gather\": \"%s\", \"rccl_version\": %s, "
                    "%s, \"per_member\": [%s], \"gather_ms\": %.4f, \"%s\": %.4f%s}\n",
                    cfg.width, cfg.height, cfg.spp, cfg.depth, app.sphere_count(), cfg.cbuffers ? "true" : "false",
                    frames, wall, st.kernel_ms, (double)st.samples / wall / 1e6, (unsigned long long)st.segments,
                    (unsigned long long)st.sphere_tests, members, devs.c_str(),
                    rtx_group_gather_mode(grp) == RTX_GATHER_RCCL ? "rccl" : "copy", rccl.c_str(), split.c_str(),
                    per.c_str(), gather_ms, split_frames ? "fold_ms" : "deinterleave_ms", deint_ms,
                    (ref + extra).c_str());
        if (!save_state.empty() && !app.SaveState(save_state)) {
            std::fprintf(stderr, "rtx_cli: --save-state failed: %s\n", app.last_error().c_str());
            return 1;
        }
    } else if (refining) {
        if (sync_rc != RTX_OK || rtx_get_stats(app.context(), &st) != RTX_OK) {
            std::fprintf(stderr, "rtx_cli: refine failed: %s\n", rtx_last_error());
            return 1;
        }
        std::string steps;
        for (size_t k = 0; k < refine.size(); ++k) steps += (k ? ", " : "") + std::to_string(refine[k]);
        for (size_t k = 0; k < ad_active.size(); ++k) steps += (k ? ", " : "") + std::to_string(ad_samples);
        for (size_t k = 0; k < mask_active.size(); ++k) steps += (steps.empty() ? "" : ", ") + std::to_string(mask_samples);
        std::vector<uint32_t> counts;
        if (adaptive || masked) {
            counts.resize((size_t)cfg.width * cfg.height);
            if (rtx_refine_counts(app.context(), counts.data(), counts.size() * sizeof(uint32_t)) != RTX_OK) {
                std::fprintf(stderr, "rtx_cli: counts failed: %s\n", rtx_last_error());
                return 1;
            }
            std::string act;
            for (size_t k = 0; k < ad_active.size(); ++k) act += (k ? ", " : "") + std::to_string(ad_active[k]);
            if (adaptive)
                std::printf("{\"refine_adaptive\": {\"samples\": %u, \"threshold\": %.9g, \"max_samples\": %u, "
                            "\"steps\": %d, \"steps_run\": %zu, \"active\": [%s]}}\n",
                            ad_samples, (double)ad_threshold, ad_max, ad_steps, ad_active.size(), act.c_str());
            if (masked) {
                std::string ids;
                for (size_t k = 0; k < mask_ids.size(); ++k) ids += (k ? ", " : "") + std::to_string(mask_ids[k]);
                for (size_t k = 0; k < mask_active.size(); ++k) act += (k ? ", " : "") + std::to_string(mask_active[k]);
                std::printf("{\"refine_masked\": {\"samples\": %u, \"ids\": [%s], \"grow\": %u, \"steps\": %d, "
                            "\"steps_run\": %zu, \"mask_pixels\": %u, \"active\": [%s]}}\n",
                            mask_samples, ids.c_str(), mask_grow, ad_steps, mask_active.size(), mask_pixels, act.c_str());
            }
            if (!dump_counts.empty()) {
                std::vector<float> img(4 * counts.size());
                for (size_t i = 0; i < counts.size(); ++i)
                    img[4 * i] = img[4 * i + 1] = img[4 * i + 2] = img[4 * i + 3] = (float)counts[i];
                if (!rtx::write_pfm(dump_counts, img.data(), cfg.width, cfg.height)) return 1;
            }
        }
        std::printf("{\"width\": %u, \"height\": %u, \"depth\": %u, \"spheres\": %u, \"cbuffers\": %s, "
                    "\"refine\": [%s], \"loaded_samples\": %u, \"refined_samples\": %u, \"wall_s\": %.6f, "
                    "\"kernel_ms\": %.4f, \"msamples_per_s\": %.3f, \"segments\": %llu, \"sphere_tests\": %llu, "
                    "\"refine_keys\": \"%s\"%s}\n",
                    cfg.width, cfg.height, cfg.depth, app.sphere_count(), cfg.cbuffers ? "true" : "false",
                    steps.c_str(), loaded_samples, rtx_refined_samples(app.context()), wall, st.kernel_ms,
                    (double)st.samples / wall / 1e6, (unsigned long long)st.segments,
                    (unsigned long long)st.sphere_tests, refine_keys == RTX_REFINE_KEYS_CARRIED ? "carried" : "prepass",
                    extra.c_str());
        if (!save_state.empty() && !app.SaveState(save_state)) {
            std::fprintf(stderr, "rtx_cli: --save-state failed: %s\n", app.last_error().c_str());
            return 1;
        }
    } else {
        rtx_get_stats(app.context(), &st);
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %u, \"depth\": %u, \"spheres\": %u, "
                    "\"cbuffers\": %s, \"frames\": %d, \"wall_s\": %.6f, \"kernel_ms\": %.4f, \"msamples_per_s\": %.3f, "
                    "\"segments\": %llu, \"sphere_tests\": %llu%s}\n",
                    cfg.width, cfg.height, cfg.spp, cfg.depth, app.sphere_count(), cfg.cbuffers ? "true" : "false",
                    frames, wall,
                    st.kernel_ms, (double)st.samples / wall / 1e6, (unsigned long long)st.segments,
                    (unsigned long long)st.sphere_tests, extra.c_str());
    }
    if (!pfm.empty() || !ppm.empty()) {
        std::vector<float> img;
        if (!app.Download(img)) {
            std::fprintf(stderr, "rtx_cli: download failed: %s\n", app.last_error().c_str());
            return 1;
        }
        if (!pfm.empty() && !rtx::write_pfm(pfm, img.data(), cfg.width, cfg.height)) return 1;
        if (!ppm.empty() && !rtx::write_ppm(ppm, img.data(), cfg.width, cfg.height)) return 1;
    }
    app.Terminate();
    return 0;
}
