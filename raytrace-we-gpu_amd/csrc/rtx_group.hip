// rtx_group.hip — one frame across several devices through the C-ABI
// (include/rtx.h rtx_group): n contexts, their buffers and the gather, driven
// by one host thread. The partition and buffer arithmetic is
// rtx_group_plan.h's; this file executes that plan on device memory with the
// single-context entry points (rtx_render_rows, rtx_deinterleave_rows).
// rtx_group_accumulate is the second split: whole progressive frames dealt to
// the members (rtx_render_sum), their sums gathered into the root's slots and
// folded in frame order (rtx_fold_frames); its plan is in the same header.
// rtx_group_refine is the row split again with rtx_refine_rows as each member's
// launch (run_frame is the body all three share): every member keeps the chain
// state of its own rows, and the group's checkpoint is one whole-frame state,
// shuffled on the host by the plan header's scatter and gather.
// rtx_group_refine_adaptive puts a phase in front of that launch: the members'
// edge rows of the error map, exchanged by the plan header's halo plan, and
// the members' masks.
//
// RCCL is loaded at run time (dlopen), so librtx.so carries no link
// dependency on it: a single-GPU user pays nothing, and a process that has
// another RCCL loaded already (torch's) gets that one.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtx.h"
#include "rtx_group_plan.h"
#include "rtx_internal.h"

namespace {

int fail(int code, const std::string &msg) { return rtx::api_fail(code, msg.c_str()); }

int hip_fail(hipError_t e, const char *what) {
    return fail(RTX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define RTXG_HIP(call)                                    \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// The part of RCCL's C interface the gather uses, declared here so that the
// build needs no RCCL header (rccl.h: ncclResult_t 0 = ncclSuccess,
// ncclFloat = 7, ncclComm_t an opaque pointer).
typedef void *nccl_comm;
constexpr int kNcclFloat = 7;
struct Rccl {
    void *handle = nullptr;
    int (*CommInitAll)(nccl_comm *, int, const int *) = nullptr;
    int (*CommDestroy)(nccl_comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, nccl_comm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, nccl_comm, hipStream_t) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};

// dlopen by soname; when the loader's search path does not reach it, beside
// the HIP runtime this library is already linked to.
int load_rccl(Rccl &r) {
    const char *soname = "librccl.so.1";
    void *h = dlopen(soname, RTLD_NOW | RTLD_LOCAL);
    std::string why;
    if (!h) {
        const char *e = dlerror();
        why = e ? e : "dlopen failed";
        Dl_info info;
        if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
            std::string p(info.dli_fname);
            const size_t slash = p.rfind('/');
            if (slash != std::string::npos) {
                p = p.substr(0, slash + 1) + soname;
                h = dlopen(p.c_str(), RTLD_NOW | RTLD_LOCAL);
            }
        }
    }
    if (!h) return fail(RTX_ERR_STATE, "rtx_group_create: RCCL not loaded: " + why);
    const struct {
        const char *name;
        void **slot;
    } syms[] = {{"ncclCommInitAll", reinterpret_cast<void **>(&r.CommInitAll)},
                {"ncclCommDestroy", reinterpret_cast<void **>(&r.CommDestroy)},
                {"ncclGroupStart", reinterpret_cast<void **>(&r.GroupStart)},
                {"ncclGroupEnd", reinterpret_cast<void **>(&r.GroupEnd)},
                {"ncclSend", reinterpret_cast<void **>(&r.Send)},
                {"ncclRecv", reinterpret_cast<void **>(&r.Recv)},
                {"ncclGetVersion", reinterpret_cast<void **>(&r.GetVersion)},
                {"ncclGetErrorString", reinterpret_cast<void **>(&r.GetErrorString)}};
    for (const auto &s : syms) {
        *s.slot = dlsym(h, s.name);
        if (!*s.slot) {
            const char *e = dlerror();
            const std::string msg = std::string("rtx_group_create: RCCL lacks ") + s.name + ": " + (e ? e : "");
            dlclose(h);
            return fail(RTX_ERR_STATE, msg);
        }
    }
    r.handle = h;
    return RTX_OK;
}

struct Member {
    int device = 0;
    rtx_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;  // the context's; members on one device share the root member's
    void *d_send = nullptr;        // its rows (members 1 .. n-1)
    size_t send_bytes = 0;
    hipEvent_t ev_start = nullptr, ev_rendered = nullptr;
    bool rendered = false;         // the last frame launched a render for it
    void *d_sum = nullptr;         // rtx_group_accumulate: its frame's sums (members 1 .. n-1)
    hipEvent_t ev_sum0 = nullptr, ev_sum1 = nullptr;
    bool summed = false;           // the last accumulate round launched a render for it
    nccl_comm comm = nullptr;
    // rtx_group_refine_adaptive: its tiles' edge rows of err and its neighbours'
    // (rtx_group_plan.h HaloPlan), the N the group expects of its chain state
    void *d_edges = nullptr, *d_halo = nullptr;
    hipEvent_t ev_edges = nullptr;
    uint32_t ref_n = 0;
};

}  // namespace

struct rtx_group {
    std::vector<Member> m;
    bool one_device = false;  // every member on the root's device (the rehearsal)
    int mode = RTX_GATHER_COPY;
    Rccl rccl;
    int rccl_version = 0;
    rtx_frame frame{};
    bool have_frame = false;
    rtx::GroupPlan plan;      // of the buffers below (n == 0: none yet)
    bool direct = false;      // one member, copies: it renders straight into the image
    void *d_gathered = nullptr;
    void *d_image = nullptr;
    hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr, ev_d0 = nullptr, ev_d1 = nullptr;
    bool launched = false;    // a frame's events are recorded
    bool gathered_once = false;
    bool have_times = false;
    std::vector<double> render_ms;
    double gather_ms = 0.0, deint_ms = 0.0;
    size_t image_pixels = 0;  // of d_image (rtx_group_render and rtx_group_accumulate share it)
    // rtx_group_accumulate
    rtx::AccumPlan aplan;     // of the buffers below (n == 0: none yet)
    void *d_accum = nullptr;  // [pixels] linear sums over acc_frames frames
    void *d_sums = nullptr;   // [n][pixels] a round's sums, slot i member i's
    uint32_t acc_frames = 0;
    hipEvent_t ev_a0 = nullptr, ev_a1 = nullptr, ev_f0 = nullptr, ev_f1 = nullptr;
    bool acc_launched = false;    // a round's events are recorded
    bool acc_gathered = false;    // ... ev_a1 among them
    bool have_acc_times = false;
    std::vector<double> acc_render_ms;
    double acc_gather_ms = 0.0, fold_ms = 0.0;
    // rtx_group_refine: the samples in the members' chain states (0: none, the
    // next call starts everyone fresh) and the tile_rows they were cut by
    uint32_t ref_n = 0, ref_tile = 0;
    // rtx_group_refine_adaptive: some call traced a proper subset (the counts
    // may differ), and the plan of the members' edge and halo buffers
    bool ref_mixed = false;
    rtx::HaloPlan hplan;
};

namespace {

int nccl_fail(const rtx_group *g, int rc, const char *what) {
    return fail(RTX_ERR_HIP, std::string(what) + ": " + g->rccl.GetErrorString(rc));
}

void free_buffers(rtx_group *g) {
    for (Member &mb : g->m) {
        if (mb.d_send) {
            (void)hipSetDevice(mb.device);
            (void)hipFree(mb.d_send);
        }
        mb.d_send = nullptr;
        mb.send_bytes = 0;
    }
    if (!g->m.empty()) (void)hipSetDevice(g->m[0].device);
    (void)hipFree(g->d_gathered);
    g->d_gathered = nullptr;
    g->plan = rtx::GroupPlan();
}

void free_accum_buffers(rtx_group *g) {
    for (Member &mb : g->m) {
        if (mb.d_sum) {
            (void)hipSetDevice(mb.device);
            (void)hipFree(mb.d_sum);
        }
        mb.d_sum = nullptr;
    }
    if (!g->m.empty()) (void)hipSetDevice(g->m[0].device);
    (void)hipFree(g->d_accum);
    (void)hipFree(g->d_sums);
    g->d_accum = g->d_sums = nullptr;
    g->aplan = rtx::AccumPlan();
    g->acc_frames = 0;
}

void free_halo_buffers(rtx_group *g) {
    for (Member &mb : g->m) {
        if (mb.d_edges || mb.d_halo) (void)hipSetDevice(mb.device);
        (void)hipFree(mb.d_edges);
        (void)hipFree(mb.d_halo);
        mb.d_edges = mb.d_halo = nullptr;
    }
    g->hplan = rtx::HaloPlan();
}

void free_image(rtx_group *g) {
    if (!g->m.empty()) (void)hipSetDevice(g->m[0].device);
    (void)hipFree(g->d_image);
    g->d_image = nullptr;
    g->image_pixels = 0;
}

// Every member's stream drained (before buffers are replaced).
int drain(rtx_group *g) {
    for (Member &mb : g->m) {
        RTXG_HIP(hipSetDevice(mb.device));
        RTXG_HIP(hipStreamSynchronize(mb.stream));
    }
    return RTX_OK;
}

// The image, width*height pixels on the root's device, shared by
// rtx_group_render and rtx_group_accumulate; the streams are drained before
// another size replaces it.
int ensure_image(rtx_group *g) {
    const size_t px = (size_t)g->frame.width * g->frame.height;
    if (g->d_image && g->image_pixels == px) return RTX_OK;
    if (g->d_image) {
        const int rc = drain(g);
        if (rc) return rc;
    }
    free_image(g);
    RTXG_HIP(hipSetDevice(g->m[0].device));
    RTXG_HIP(hipMalloc(&g->d_image, px * rtx::kGroupPixelBytes));
    g->image_pixels = px;
    return RTX_OK;
}

// Buffers for this frame size and tile_rows (render_impl's treatment of d_fb:
// another size drains the streams and replaces them).
int ensure_buffers(rtx_group *g, uint32_t tile_rows) {
    const uint32_t n = (uint32_t)g->m.size();
    // (the image follows the frame size on its own: rtx_group_accumulate may have replaced it)
    int rc = ensure_image(g);
    if (rc) return rc;
    if (g->plan.same(n, g->frame.width, g->frame.height, tile_rows)) return RTX_OK;
    rc = drain(g);
    if (rc) return rc;
    free_buffers(g);
    g->gathered_once = false;
    const rtx::GroupPlan plan = rtx::make_group_plan(n, g->frame.width, g->frame.height, tile_rows);
    g->direct = n == 1 && g->mode == RTX_GATHER_COPY;
    RTXG_HIP(hipSetDevice(g->m[0].device));
    if (!g->direct) RTXG_HIP(hipMalloc(&g->d_gathered, plan.gathered_bytes));
    for (uint32_t i = 1; i < n; ++i) {
        Member &mb = g->m[i];
        RTXG_HIP(hipSetDevice(mb.device));
        // a member without rows keeps a (small) buffer: the collective names it
        RTXG_HIP(hipMalloc(&mb.d_send, plan.send_bytes[i] ? plan.send_bytes[i] : rtx::kGroupPixelBytes));
        mb.send_bytes = plan.send_bytes[i];
    }
    g->plan = plan;
    return RTX_OK;
}

// rtx_group_accumulate's buffers for this frame size: the accumulator, the
// root's n sum slots and one sum buffer per other member.
int ensure_accum_buffers(rtx_group *g) {
    const uint32_t n = (uint32_t)g->m.size();
    int rc = ensure_image(g);  // (rtx_group_render may have replaced it for another size)
    if (rc) return rc;
    if (g->aplan.same(n, g->frame.width, g->frame.height) && g->d_accum) return RTX_OK;
    rc = drain(g);
    if (rc) return rc;
    free_accum_buffers(g);
    g->acc_gathered = false;
    const rtx::AccumPlan plan = rtx::make_accum_plan(n, g->frame.width, g->frame.height);
    RTXG_HIP(hipSetDevice(g->m[0].device));
    RTXG_HIP(hipMalloc(&g->d_accum, plan.slot_bytes));
    RTXG_HIP(hipMalloc(&g->d_sums, plan.sums_bytes));
    for (uint32_t i = 1; i < n; ++i) {
        Member &mb = g->m[i];
        RTXG_HIP(hipSetDevice(mb.device));
        RTXG_HIP(hipMalloc(&mb.d_sum, plan.slot_bytes));
    }
    g->aplan = plan;
    return RTX_OK;
}

void destroy_group(rtx_group *g) {
    for (Member &mb : g->m) {
        if (!mb.ctx) continue;
        (void)hipSetDevice(mb.device);
        (void)hipStreamSynchronize(mb.stream);
    }
    for (Member &mb : g->m)
        if (mb.comm) (void)g->rccl.CommDestroy(mb.comm);
    free_buffers(g);
    free_accum_buffers(g);
    free_halo_buffers(g);
    free_image(g);
    if (!g->m.empty() && g->m[0].ctx) (void)hipSetDevice(g->m[0].device);
    for (hipEvent_t e : {g->ev_g0, g->ev_g1, g->ev_d0, g->ev_d1, g->ev_a0, g->ev_a1, g->ev_f0, g->ev_f1})
        if (e) (void)hipEventDestroy(e);
    // the root last: the members on its device launch on its stream
    for (size_t i = g->m.size(); i-- > 0;) {
        Member &mb = g->m[i];
        if (!mb.ctx) continue;
        (void)hipSetDevice(mb.device);
        if (mb.ev_start) (void)hipEventDestroy(mb.ev_start);
        if (mb.ev_rendered) (void)hipEventDestroy(mb.ev_rendered);
        if (mb.ev_sum0) (void)hipEventDestroy(mb.ev_sum0);
        if (mb.ev_sum1) (void)hipEventDestroy(mb.ev_sum1);
        if (mb.ev_edges) (void)hipEventDestroy(mb.ev_edges);
        (void)rtx_use_own_stream(mb.ctx);
        rtx_destroy(mb.ctx);
    }
    // the RCCL handle stays loaded: its communicators' teardown may outlive this call
    delete g;
}

// One frame of the row split into the image: every row-owning member's launch
// (launch(i, n, d_out): member i's rows into d_out, asynchronous on its
// stream), the gather, then the de-interleave on the root's stream.
// rtx_group_render, rtx_group_refine and rtx_group_refine_import differ in the
// launch only. The buffers fit (ensure_buffers).
template <class Launch>
int run_frame(rtx_group *g, const char *fn, Launch launch) {
    int rc = RTX_OK;
    const rtx::GroupPlan &plan = g->plan;
    const uint32_t n = plan.n;
    Member &root = g->m[0];
    g->have_times = false;

    // every member's render, one after the other from this thread: each is
    // asynchronous on its member's stream
    for (uint32_t i = 0; i < n; ++i) {
        Member &mb = g->m[i];
        mb.rendered = false;
        if (!plan.renders(i)) continue;
        RTXG_HIP(hipSetDevice(mb.device));
        // its send buffer is free once the root has pulled the last frame's rows
        if (i > 0 && !g->one_device && g->mode == RTX_GATHER_COPY && g->gathered_once)
            RTXG_HIP(hipStreamWaitEvent(mb.stream, g->ev_g1, 0));
        void *d_out = i > 0 ? mb.d_send : (g->direct ? g->d_image : g->d_gathered);
        RTXG_HIP(hipEventRecord(mb.ev_start, mb.stream));
        rc = launch(i, n, d_out);
        if (rc != RTX_OK) {
            const std::string why = rtx_last_error();
            return fail(rc, std::string(fn) + ": member " + std::to_string(i) + ": " + why);
        }
        RTXG_HIP(hipSetDevice(mb.device));
        RTXG_HIP(hipEventRecord(mb.ev_rendered, mb.stream));
        mb.rendered = true;
    }

    // the gather, on the root's stream
    RTXG_HIP(hipSetDevice(root.device));
    RTXG_HIP(hipEventRecord(g->ev_g0, root.stream));
    if (g->mode == RTX_GATHER_COPY) {
        for (const rtx::GroupOp &op : plan.ops) {
            if (op.bytes == 0) continue;
            Member &mb = g->m[op.member];
            char *dst = static_cast<char *>(g->d_gathered) + op.dst_off;
            RTXG_HIP(hipStreamWaitEvent(root.stream, mb.ev_rendered, 0));
            if (mb.device == root.device)
                RTXG_HIP(hipMemcpyAsync(dst, mb.d_send, op.bytes, hipMemcpyDeviceToDevice, root.stream));
            else
                RTXG_HIP(hipMemcpyPeerAsync(dst, root.device, mb.d_send, mb.device, op.bytes, root.stream));
        }
    } else {
        // what ncclGather does inside, with the symbols every RCCL has
        int nrc = g->rccl.GroupStart();
        if (nrc != 0) return nccl_fail(g, nrc, (std::string(fn) + ": ncclGroupStart").c_str());
        for (const rtx::GroupOp &op : plan.ops) {
            Member &mb = g->m[op.member];
            const size_t floats = op.bytes / sizeof(float);
            char *dst = static_cast<char *>(g->d_gathered) + op.dst_off;
            (void)hipSetDevice(mb.device);
            if (nrc == 0) nrc = g->rccl.Send(mb.d_send, floats, kNcclFloat, 0, mb.comm, mb.stream);
            (void)hipSetDevice(root.device);
            if (nrc == 0) nrc = g->rccl.Recv(dst, floats, kNcclFloat, (int)op.member, root.comm, root.stream);
        }
        const int erc = g->rccl.GroupEnd();  // always closed, also after a failed call inside
        if (nrc != 0) return nccl_fail(g, nrc, (std::string(fn) + ": ncclSend/ncclRecv").c_str());
        if (erc != 0) return nccl_fail(g, erc, (std::string(fn) + ": ncclGroupEnd").c_str());
        RTXG_HIP(hipSetDevice(root.device));
    }
    RTXG_HIP(hipEventRecord(g->ev_g1, root.stream));
    g->gathered_once = true;

    // the de-interleave, after the gather on the same stream
    RTXG_HIP(hipEventRecord(g->ev_d0, root.stream));
    if (!g->direct) {
        rc = rtx_deinterleave_rows(root.ctx, g->d_gathered, plan.width, plan.height, plan.tile_rows, n, g->d_image);
        if (rc != RTX_OK) return rc;
        RTXG_HIP(hipSetDevice(root.device));
    }
    RTXG_HIP(hipEventRecord(g->ev_d1, root.stream));
    g->launched = true;
    return RTX_OK;
}

}  // namespace

extern "C" {

int rtx_group_create(const int *devices, uint32_t n, int gather_mode, rtx_group **out) {
    // arguments first: nothing below this block runs for a bad one, and
    // nothing in it touches HIP
    if (!out) return fail(RTX_ERR_INVALID, "rtx_group_create: null out");
    *out = nullptr;
    if (!devices) return fail(RTX_ERR_INVALID, "rtx_group_create: null devices");
    if (n == 0) return fail(RTX_ERR_INVALID, "rtx_group_create: n is 0");
    if (n > RTX_GROUP_MAX)
        return fail(RTX_ERR_INVALID, "rtx_group_create: n " + std::to_string(n) + " above RTX_GROUP_MAX (" +
                                         std::to_string(RTX_GROUP_MAX) + ")");
    if (gather_mode != RTX_GATHER_AUTO && gather_mode != RTX_GATHER_RCCL && gather_mode != RTX_GATHER_COPY)
        return fail(RTX_ERR_INVALID, "rtx_group_create: unknown gather_mode " + std::to_string(gather_mode));
    bool all_equal = true, all_distinct = true;
    for (uint32_t i = 0; i < n; ++i) {
        if (devices[i] < 0)
            return fail(RTX_ERR_INVALID, "rtx_group_create: devices[" + std::to_string(i) + "] is negative");
        if (devices[i] != devices[0]) all_equal = false;
        for (uint32_t j = 0; j < i; ++j)
            if (devices[j] == devices[i]) all_distinct = false;
    }
    if (!all_equal && !all_distinct)
        return fail(RTX_ERR_INVALID, "rtx_group_create: devices must be all distinct or all equal (the one-GPU "
                                     "rehearsal)");
    if (gather_mode == RTX_GATHER_RCCL && !all_distinct)
        return fail(RTX_ERR_INVALID, "rtx_group_create: gather_mode RTX_GATHER_RCCL needs distinct devices");

    rtx_group *g = new (std::nothrow) rtx_group();
    if (!g) return fail(RTX_ERR_NOMEM, "rtx_group_create: out of host memory");
    g->one_device = all_equal;
    g->mode = gather_mode == RTX_GATHER_AUTO ? (all_equal ? RTX_GATHER_COPY : RTX_GATHER_RCCL) : gather_mode;
    g->m.resize(n);
    g->render_ms.assign(n, 0.0);
    g->acc_render_ms.assign(n, 0.0);
    int rc = RTX_OK;
    hipError_t e = hipSuccess;
    for (uint32_t i = 0; i < n && rc == RTX_OK; ++i) {
        Member &mb = g->m[i];
        mb.device = devices[i];
        rc = rtx_create(mb.device, &mb.ctx);
        if (rc != RTX_OK) {
            mb.ctx = nullptr;
            const std::string why = rtx_last_error();
            fail(rc, "rtx_group_create: member " + std::to_string(i) + ": " + why);
            break;
        }
        // one stream per device: two persistent renders must not compete for
        // one device's resident waves, so the rehearsal's members queue up
        if (i > 0 && all_equal) rc = rtx_set_stream(mb.ctx, g->m[0].stream);
        mb.stream = rtx::ctx_stream(mb.ctx);
        e = hipSetDevice(mb.device);
        if (e == hipSuccess) e = hipEventCreate(&mb.ev_start);
        if (e == hipSuccess) e = hipEventCreate(&mb.ev_rendered);
        if (e == hipSuccess) e = hipEventCreate(&mb.ev_sum0);
        if (e == hipSuccess) e = hipEventCreate(&mb.ev_sum1);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mb.ev_edges, hipEventDisableTiming);
        if (e != hipSuccess) rc = hip_fail(e, "rtx_group_create: hipEventCreate");
    }
    if (rc == RTX_OK) {
        e = hipSetDevice(g->m[0].device);
        for (hipEvent_t *ev : {&g->ev_g0, &g->ev_g1, &g->ev_d0, &g->ev_d1, &g->ev_a0, &g->ev_a1, &g->ev_f0, &g->ev_f1})
            if (e == hipSuccess) e = hipEventCreate(ev);
        if (e != hipSuccess) rc = hip_fail(e, "rtx_group_create: hipEventCreate");
    }
    if (rc == RTX_OK && g->mode == RTX_GATHER_COPY && !all_equal) {
        // direct peer copies where the devices allow them (hipMemcpyPeerAsync
        // stages through the host otherwise)
        for (uint32_t i = 1; i < n; ++i) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, g->m[0].device, g->m[i].device) == hipSuccess && can)
                (void)hipDeviceEnablePeerAccess(g->m[i].device, 0);
            (void)hipGetLastError();  // "already enabled" is no failure
        }
    }
    if (rc == RTX_OK && g->mode == RTX_GATHER_RCCL) {
        rc = load_rccl(g->rccl);
        if (rc == RTX_OK) {
            (void)g->rccl.GetVersion(&g->rccl_version);
            std::vector<nccl_comm> comms(n, nullptr);
            const int nrc = g->rccl.CommInitAll(comms.data(), (int)n, devices);
            if (nrc != 0) rc = nccl_fail(g, nrc, "rtx_group_create: ncclCommInitAll");
            else
                for (uint32_t i = 0; i < n; ++i) g->m[i].comm = comms[i];
        }
    }
    if (rc != RTX_OK) {
        const std::string why = rtx_last_error();
        destroy_group(g);
        return fail(rc, why);
    }
    *out = g;
    return RTX_OK;
}

void rtx_group_destroy(rtx_group *g) {
    if (g) destroy_group(g);
}

uint32_t rtx_group_size(rtx_group *g) { return g ? (uint32_t)g->m.size() : 0; }

rtx_ctx *rtx_group_ctx(rtx_group *g, uint32_t member) {
    return (g && member < g->m.size()) ? g->m[member].ctx : nullptr;
}

int rtx_group_gather_mode(rtx_group *g) { return g ? g->mode : RTX_GATHER_AUTO; }

int rtx_group_rccl_version(rtx_group *g) { return g ? g->rccl_version : 0; }

int rtx_group_upload_world(rtx_group *g, const rtx_world *w) {
    if (!g || !w) return fail(RTX_ERR_INVALID, "rtx_group_upload_world: null argument");
    g->ref_n = 0;  // a chain state belongs to its world (as every member's falls)
    for (size_t i = 0; i < g->m.size(); ++i) {
        const int rc = rtx_upload_world(g->m[i].ctx, w);
        if (rc != RTX_OK) {
            const std::string why = rtx_last_error();
            return fail(rc, "rtx_group_upload_world: member " + std::to_string(i) + ": " + why);
        }
    }
    return RTX_OK;
}

int rtx_group_set_frame(rtx_group *g, const rtx_frame *f) {
    if (!g || !f) return fail(RTX_ERR_INVALID, "rtx_group_set_frame: null argument");
    // ... and to its frame: other bytes restart it, the same bytes again keep it
    if (!g->have_frame || std::memcmp(f, &g->frame, sizeof *f) != 0) g->ref_n = 0;
    for (size_t i = 0; i < g->m.size(); ++i) {
        const int rc = rtx_set_frame(g->m[i].ctx, f);
        if (rc != RTX_OK) {
            const std::string why = rtx_last_error();
            return fail(rc, "rtx_group_set_frame: member " + std::to_string(i) + ": " + why);
        }
    }
    g->frame = *f;
    g->have_frame = true;
    return RTX_OK;
}

int rtx_group_render(rtx_group *g, uint32_t tile_rows) {
    if (!g) return fail(RTX_ERR_INVALID, "rtx_group_render: null group");
    if (tile_rows == 0) return fail(RTX_ERR_INVALID, "rtx_group_render: tile_rows is 0");
    if (!g->have_frame) return fail(RTX_ERR_STATE, "rtx_group_render: no frame set");
    const int rc = ensure_buffers(g, tile_rows);
    if (rc) return rc;
    return run_frame(g, "rtx_group_render", [&](uint32_t i, uint32_t n, void *d_out) {
        return rtx_render_rows(g->m[i].ctx, tile_rows, i, n, d_out);
    });
}

int rtx_group_accumulate(rtx_group *g, uint32_t frames, int reset) {
    // arguments and state first: nothing in this block touches HIP
    if (!g) return fail(RTX_ERR_INVALID, "rtx_group_accumulate: null group");
    if (frames == 0) return fail(RTX_ERR_INVALID, "rtx_group_accumulate: frames is 0");
    if (!g->have_frame) return fail(RTX_ERR_STATE, "rtx_group_accumulate: no frame set");
    const uint32_t n = (uint32_t)g->m.size();
    uint32_t spp = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t s = 0;
        if (!rtx::ctx_world_spp(g->m[i].ctx, &s))
            return fail(RTX_ERR_STATE, "rtx_group_accumulate: member " + std::to_string(i) + ": no world uploaded");
        if (i > 0 && s != spp)
            return fail(RTX_ERR_STATE, "rtx_group_accumulate: member " + std::to_string(i) + ": another spp than the root's");
        spp = s;
    }
    if (spp == 0) return fail(RTX_ERR_INVALID, "rtx_group_accumulate: spp is 0 (no divisor)");
    // a frame of another size restarts the accumulation, as rtx_accumulate does
    const bool restart = reset || g->acc_frames == 0 || !g->d_accum ||
                         !g->aplan.same(n, g->frame.width, g->frame.height);
    const uint32_t first = restart ? 0u : g->acc_frames;
    if (!rtx::accum_call_valid(first, frames, spp))
        return fail(RTX_ERR_INVALID, "rtx_group_accumulate: " + std::to_string(first) + " + " + std::to_string(frames) +
                                         " frames of " + std::to_string(spp) +
                                         " spp: frame_index above 0x7fffffff or frames * spp above 2^32 - 1");

    int rc = ensure_accum_buffers(g);
    if (rc) return rc;
    const rtx::AccumPlan &plan = g->aplan;
    Member &root = g->m[0];
    if (restart) {
        RTXG_HIP(hipSetDevice(root.device));
        RTXG_HIP(hipMemsetAsync(g->d_accum, 0, plan.slot_bytes, root.stream));
        g->acc_frames = 0;
    }
    g->have_acc_times = false;

    const uint32_t rounds = rtx::accum_rounds(n, frames);
    for (uint32_t r = 0; r < rounds; ++r) {
        const rtx::AccumRound round = rtx::accum_round(plan, first, frames, spp, r);
        // the round's frames, one per taking member, each asynchronous on its member's stream
        for (uint32_t i = 0; i < n; ++i) {
            Member &mb = g->m[i];
            mb.summed = false;
            if (!round.takes(i)) continue;
            RTXG_HIP(hipSetDevice(mb.device));
            // its sum buffer is free once the root has pulled the last round's sums
            if (i > 0 && !g->one_device && g->mode == RTX_GATHER_COPY && g->acc_gathered)
                RTXG_HIP(hipStreamWaitEvent(mb.stream, g->ev_a1, 0));
            void *d_out = i > 0 ? mb.d_sum : g->d_sums;  // the root: slot 0
            RTXG_HIP(hipEventRecord(mb.ev_sum0, mb.stream));
            rc = rtx_render_sum(mb.ctx, round.frame_index(i), d_out);
            if (rc != RTX_OK) {
                const std::string why = rtx_last_error();
                return fail(rc, "rtx_group_accumulate: member " + std::to_string(i) + ": " + why);
            }
            RTXG_HIP(hipSetDevice(mb.device));
            RTXG_HIP(hipEventRecord(mb.ev_sum1, mb.stream));
            mb.summed = true;
        }
        // the gather into slots 1 .. m-1, on the root's stream
        RTXG_HIP(hipSetDevice(root.device));
        RTXG_HIP(hipEventRecord(g->ev_a0, root.stream));
        if (g->mode == RTX_GATHER_COPY) {
            for (const rtx::GroupOp &op : round.ops) {
                Member &mb = g->m[op.member];
                char *dst = static_cast<char *>(g->d_sums) + op.dst_off;
                RTXG_HIP(hipStreamWaitEvent(root.stream, mb.ev_sum1, 0));
                if (mb.device == root.device)
                    RTXG_HIP(hipMemcpyAsync(dst, mb.d_sum, op.bytes, hipMemcpyDeviceToDevice, root.stream));
                else
                    RTXG_HIP(hipMemcpyPeerAsync(dst, root.device, mb.d_sum, mb.device, op.bytes, root.stream));
            }
        } else if (!round.ops.empty()) {
            int nrc = g->rccl.GroupStart();
            if (nrc != 0) return nccl_fail(g, nrc, "rtx_group_accumulate: ncclGroupStart");
            for (const rtx::GroupOp &op : round.ops) {
                Member &mb = g->m[op.member];
                const size_t floats = op.bytes / sizeof(float);
                char *dst = static_cast<char *>(g->d_sums) + op.dst_off;
                (void)hipSetDevice(mb.device);
                if (nrc == 0) nrc = g->rccl.Send(mb.d_sum, floats, kNcclFloat, 0, mb.comm, mb.stream);
                (void)hipSetDevice(root.device);
                if (nrc == 0) nrc = g->rccl.Recv(dst, floats, kNcclFloat, (int)op.member, root.comm, root.stream);
            }
            const int erc = g->rccl.GroupEnd();  // always closed, also after a failed call inside
            if (nrc != 0) return nccl_fail(g, nrc, "rtx_group_accumulate: ncclSend/ncclRecv");
            if (erc != 0) return nccl_fail(g, erc, "rtx_group_accumulate: ncclGroupEnd");
            RTXG_HIP(hipSetDevice(root.device));
        }
        RTXG_HIP(hipEventRecord(g->ev_a1, root.stream));
        g->acc_gathered = true;

        // the fold of slots 0 .. m-1 (member order = frame order), after the gather on the same stream
        RTXG_HIP(hipEventRecord(g->ev_f0, root.stream));
        rc = rtx_fold_frames(root.ctx, g->d_accum, g->d_sums, round.m, plan.pixels, plan.pixels, round.divisor,
                             g->d_image);
        if (rc != RTX_OK) return rc;
        RTXG_HIP(hipSetDevice(root.device));
        RTXG_HIP(hipEventRecord(g->ev_f1, root.stream));
        g->acc_frames = round.frames_after;
        g->acc_launched = true;
    }
    return RTX_OK;
}

uint32_t rtx_group_accumulated_frames(rtx_group *g) { return g ? g->acc_frames : 0; }

// ---- progressive refinement across the members ------------------------------
namespace {

// What rtx_group_refine and rtx_group_refine_import decide before any HIP call.
int refine_call_check(rtx_group *g, const char *fn, uint32_t samples, uint32_t tile_rows) {
    const std::string f(fn);
    if (!g) return fail(RTX_ERR_INVALID, f + ": null group");
    if (samples == 0) return fail(RTX_ERR_INVALID, f + ": samples is 0");
    if (tile_rows == 0) return fail(RTX_ERR_INVALID, f + ": tile_rows is 0");
    if (!g->have_frame) return fail(RTX_ERR_STATE, f + ": no frame set");
    for (size_t i = 0; i < g->m.size(); ++i) {
        uint32_t spp = 0;
        if (!rtx::ctx_world_spp(g->m[i].ctx, &spp))
            return fail(RTX_ERR_STATE, f + ": member " + std::to_string(i) + ": no world uploaded");
    }
    if (g->frame.rng_mode == RTX_RNG_PER_SAMPLE)
        return fail(RTX_ERR_INVALID, f + ": the per-sample RNG has no chain to continue (rtx_group_accumulate is its "
                                         "progressive form)");
    return RTX_OK;
}

// Every row-owning member's chain state is the group's: the member's ref_n
// samples (the group's, unless an adaptive step traced nothing of its rows) of
// part i of n in tiles of ref_tile rows. Anything else means someone refined
// through a borrowed rtx_group_ctx.
int members_agree(rtx_group *g, const char *fn) {
    const uint32_t n = (uint32_t)g->m.size();
    for (uint32_t i = 0; i < n; ++i) {
        if (rtx::group_part_rows(g->frame.height, g->ref_tile, i, n) == 0) continue;
        uint32_t t = 0, part = 0, np = 0;
        const uint32_t have = rtx_refined_samples(g->m[i].ctx);
        const bool shaped = rtx_refine_shape(g->m[i].ctx, &t, &part, &np) == RTX_OK;
        const uint32_t want_t = n == 1 ? 1u : g->ref_tile;  // (a whole frame's shape is (1, 0, 1))
        if (have != g->m[i].ref_n || !shaped || t != want_t || part != i || np != n)
            return fail(RTX_ERR_STATE, std::string(fn) + ": member " + std::to_string(i) + ": its chain state (" +
                                           std::to_string(have) + " samples) is not the group's (" +
                                           std::to_string(g->m[i].ref_n) + " samples, part " + std::to_string(i) + " of " +
                                           std::to_string(n) + " in tiles of " + std::to_string(g->ref_tile) +
                                           " rows): it was refined through rtx_group_ctx; reset the group's refine");
    }
    return RTX_OK;
}

}  // namespace

int rtx_group_refine(rtx_group *g, uint32_t samples, uint32_t tile_rows, int reset) {
    // arguments and state first: nothing in this block touches HIP
    int rc = refine_call_check(g, "rtx_group_refine", samples, tile_rows);
    if (rc) return rc;
    const bool fresh = reset || g->ref_n == 0 || g->ref_tile != tile_rows;
    const uint32_t have = fresh ? 0u : g->ref_n;
    if (samples > 0xffffffffu - have)
        return fail(RTX_ERR_INVALID, "rtx_group_refine: more than 2^32 - 1 samples in all");
    if (!fresh && g->ref_mixed)
        return fail(RTX_ERR_STATE, "rtx_group_refine: the state's per-pixel sample counts differ after adaptive steps: "
                                   "continue with rtx_group_refine_adaptive, or reset");
    if (!fresh) {
        rc = members_agree(g, "rtx_group_refine");
        if (rc) return rc;
    }
    rc = ensure_buffers(g, tile_rows);
    if (rc) return rc;
    // the group decides freshness and every member follows it; N counts again
    // only once every member's launch and the assembly are enqueued
    g->ref_n = 0;
    g->ref_mixed = false;
    rc = run_frame(g, "rtx_group_refine", [&](uint32_t i, uint32_t n, void *d_out) {
        return rtx_refine_rows(g->m[i].ctx, tile_rows, i, n, samples, fresh ? 1 : 0, d_out);
    });
    if (rc != RTX_OK) return rc;
    g->ref_n = have + samples;
    g->ref_tile = tile_rows;
    for (Member &mb : g->m) mb.ref_n = g->ref_n;
    return RTX_OK;
}

uint32_t rtx_group_refined_samples(rtx_group *g) { return g ? g->ref_n : 0; }

int rtx_group_refine_export(rtx_group *g, float *host_state, size_t bytes) {
    if (!g || !host_state) return fail(RTX_ERR_INVALID, "rtx_group_refine_export: null argument");
    if (g->ref_n == 0 || !g->have_frame) return fail(RTX_ERR_STATE, "rtx_group_refine_export: no chain state");
    const uint32_t n = (uint32_t)g->m.size();
    // (its own plan: rtx_group_render may have cut the buffers by another tile_rows since)
    const rtx::GroupPlan plan = rtx::make_group_plan(n, g->frame.width, g->frame.height, g->ref_tile);
    if (bytes != plan.image_bytes) return fail(RTX_ERR_INVALID, "rtx_group_refine_export: bytes != width*height*16");
    int rc = members_agree(g, "rtx_group_refine_export");
    if (rc) return rc;
    std::vector<std::vector<float>> parts(n);
    std::vector<const void *> ptrs(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        if (!plan.renders(i)) continue;
        const size_t part_bytes = (size_t)plan.rows[i] * plan.width * rtx::kGroupPixelBytes;
        parts[i].resize(part_bytes / sizeof(float));
        rc = rtx_refine_export(g->m[i].ctx, parts[i].data(), part_bytes);
        if (rc != RTX_OK) {
            const std::string why = rtx_last_error();
            return fail(rc, "rtx_group_refine_export: member " + std::to_string(i) + ": " + why);
        }
        ptrs[i] = parts[i].data();
    }
    rtx::group_gather_state(plan, ptrs.data(), host_state);
    return RTX_OK;
}

int rtx_group_refine_import(rtx_group *g, uint32_t tile_rows, const float *host_state, size_t bytes,
                            uint32_t samples) {
    int rc = refine_call_check(g, "rtx_group_refine_import", samples, tile_rows);
    if (rc) return rc;
    if (!host_state) return fail(RTX_ERR_INVALID, "rtx_group_refine_import: null host_state");
    if (bytes != (size_t)g->frame.width * g->frame.height * rtx::kGroupPixelBytes)
        return fail(RTX_ERR_INVALID, "rtx_group_refine_import: bytes != width*height*16");
    rc = ensure_buffers(g, tile_rows);
    if (rc) return rc;
    const rtx::GroupPlan &plan = g->plan;
    const uint32_t n = plan.n;
    std::vector<std::vector<float>> parts(n);
    std::vector<void *> ptrs(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        parts[i].resize((size_t)plan.rows[i] * plan.width * (rtx::kGroupPixelBytes / sizeof(float)));
        ptrs[i] = parts[i].data();
    }
    rtx::group_scatter_state(plan, host_state, ptrs.data());
    g->ref_n = 0;
    // each member's rows, its image rows into its slot; then the image is assembled
    rc = run_frame(g, "rtx_group_refine_import", [&](uint32_t i, uint32_t np, void *d_out) {
        return rtx_refine_import_rows(g->m[i].ctx, tile_rows, i, np, parts[i].data(), parts[i].size() * sizeof(float),
                                      samples, d_out);
    });
    if (rc != RTX_OK) return rc;
    rc = rtx_group_sync(g);  // synchronous, like rtx_refine_import
    if (rc != RTX_OK) return rc;
    g->ref_n = samples;
    g->ref_tile = tile_rows;
    g->ref_mixed = false;  // an installed state is uniform
    for (Member &mb : g->m) mb.ref_n = samples;
    return RTX_OK;
}

// ---- adaptive refinement across the members ----------------------------------
namespace {

// The members' edge and halo buffers for this frame and tile_rows (none for a
// one-member group: its rule reads the local map).
int ensure_halo_buffers(rtx_group *g, uint32_t tile_rows) {
    const uint32_t n = (uint32_t)g->m.size();
    if (g->hplan.same(n, g->frame.width, g->frame.height, tile_rows)) return RTX_OK;
    int rc = drain(g);
    if (rc) return rc;
    free_halo_buffers(g);
    const rtx::HaloPlan plan = rtx::make_halo_plan(n, g->frame.width, g->frame.height, tile_rows);
    for (uint32_t i = 0; n > 1 && i < n; ++i) {
        Member &mb = g->m[i];
        RTXG_HIP(hipSetDevice(mb.device));
        // a member without rows keeps (small) buffers: nothing names them
        const size_t bytes = plan.buffer_bytes(i) ? plan.buffer_bytes(i) : sizeof(float);
        RTXG_HIP(hipMalloc(&mb.d_edges, bytes));
        RTXG_HIP(hipMalloc(&mb.d_halo, bytes));
    }
    g->hplan = plan;
    return RTX_OK;
}

// What rtx_group_refine_adaptive and rtx_group_refine_pending decide before any HIP call.
int adaptive_call_check(rtx_group *g, const char *fn, uint32_t samples, float threshold, uint32_t max_samples,
                        uint32_t tile_rows) {
    const std::string f(fn);
    if (!g) return fail(RTX_ERR_INVALID, f + ": null group");
    if (const char *why = rtx::adaptive_args_error(samples, threshold, max_samples)) return fail(RTX_ERR_INVALID, f + ": " + why);
    const int rc = refine_call_check(g, fn, samples, tile_rows);
    if (rc) return rc;
    for (size_t i = 0; i < g->m.size(); ++i)
        if (const char *why = rtx::ctx_adaptive_refusal(g->m[i].ctx, samples))
            return fail(RTX_ERR_INVALID, f + ": member " + std::to_string(i) + ": " + why);
    return RTX_OK;
}

// Phase 1: the members' edges, the exchange, the members' masks. act[i]: the
// pixels member i would trace. A fresh call traces everything and exchanges
// nothing (every err is +inf, and max_samples >= samples).
int adaptive_phase1(rtx_group *g, const char *fn, uint32_t samples, float threshold, uint32_t max_samples,
                    uint32_t tile_rows, bool fresh, std::vector<uint32_t> &act) {
    const uint32_t n = (uint32_t)g->m.size();
    act.assign(n, 0u);
    if (fresh) {
        for (uint32_t i = 0; i < n; ++i)
            act[i] = rtx::group_part_rows(g->frame.height, tile_rows, i, n) * g->frame.width;
        return RTX_OK;
    }
    int rc = members_agree(g, fn);
    if (rc) return rc;
    rc = ensure_halo_buffers(g, tile_rows);
    if (rc) return rc;
    const rtx::HaloPlan &hp = g->hplan;
    auto member_fail = [&](int code, uint32_t i) {
        const std::string why = rtx_last_error();
        return fail(code, std::string(fn) + ": member " + std::to_string(i) + ": " + why);
    };
    if (n > 1) {
        for (uint32_t i = 0; i < n; ++i) {
            Member &mb = g->m[i];
            if (hp.tiles[i] == 0) continue;
            rc = rtx_refine_edges(mb.ctx, mb.d_edges);
            if (rc != RTX_OK) return member_fail(rc, i);
            RTXG_HIP(hipSetDevice(mb.device));
            RTXG_HIP(hipEventRecord(mb.ev_edges, mb.stream));
        }
        if (g->mode == RTX_GATHER_COPY) {
            // into each receiver's halo on the receiver's stream, after the sender's pack
            for (const rtx::HaloOp &op : hp.ops) {
                Member &src = g->m[op.src], &dst = g->m[op.dst];
                const char *from = static_cast<const char *>(src.d_edges) + op.src_off;
                char *to = static_cast<char *>(dst.d_halo) + op.dst_off;
                RTXG_HIP(hipSetDevice(dst.device));
                if (src.stream != dst.stream) RTXG_HIP(hipStreamWaitEvent(dst.stream, src.ev_edges, 0));
                if (src.device == dst.device)
                    RTXG_HIP(hipMemcpyAsync(to, from, op.bytes, hipMemcpyDeviceToDevice, dst.stream));
                else
                    RTXG_HIP(hipMemcpyPeerAsync(to, dst.device, from, src.device, op.bytes, dst.stream));
            }
        } else if (!hp.ops.empty()) {
            int nrc = g->rccl.GroupStart();
            if (nrc != 0) return nccl_fail(g, nrc, (std::string(fn) + ": ncclGroupStart").c_str());
            for (const rtx::HaloOp &op : hp.ops) {
                Member &src = g->m[op.src], &dst = g->m[op.dst];
                const size_t floats = op.bytes / sizeof(float);
                (void)hipSetDevice(src.device);
                if (nrc == 0)
                    nrc = g->rccl.Send(static_cast<const char *>(src.d_edges) + op.src_off, floats, kNcclFloat, (int)op.dst,
                                       src.comm, src.stream);
                (void)hipSetDevice(dst.device);
                if (nrc == 0)
                    nrc = g->rccl.Recv(static_cast<char *>(dst.d_halo) + op.dst_off, floats, kNcclFloat, (int)op.src,
                                       dst.comm, dst.stream);
            }
            const int erc = g->rccl.GroupEnd();  // always closed, also after a failed call inside
            if (nrc != 0) return nccl_fail(g, nrc, (std::string(fn) + ": ncclSend/ncclRecv").c_str());
            if (erc != 0) return nccl_fail(g, erc, (std::string(fn) + ": ncclGroupEnd").c_str());
        }
    }
    // every member's mask; its 4-byte count comes back (one small sync each)
    for (uint32_t i = 0; i < n; ++i) {
        Member &mb = g->m[i];
        if (hp.tiles[i] == 0) continue;
        rc = rtx_refine_pending_rows(mb.ctx, tile_rows, i, n, samples, threshold, max_samples, mb.d_halo, &act[i]);
        if (rc != RTX_OK) return member_fail(rc, i);
    }
    return RTX_OK;
}

bool adaptive_fresh(const rtx_group *g, uint32_t tile_rows, int reset) {
    return reset || g->ref_n == 0 || g->ref_tile != tile_rows;
}

// rtx_group_refine_counts / _error: the members' maps (which: 0 / 1) as one
// whole-frame map, assembled on the host.
int group_read(rtx_group *g, const char *fn, int which, void *host, size_t bytes) {
    const std::string f(fn);
    if (!g || !host) return fail(RTX_ERR_INVALID, f + ": null argument");
    if (g->ref_n == 0 || !g->have_frame) return fail(RTX_ERR_STATE, f + ": no chain state");
    const uint32_t n = (uint32_t)g->m.size();
    const rtx::GroupPlan plan = rtx::make_group_plan(n, g->frame.width, g->frame.height, g->ref_tile);
    if (bytes != (size_t)plan.width * plan.height * sizeof(uint32_t))
        return fail(RTX_ERR_INVALID, f + ": bytes != width*height*4");
    int rc = members_agree(g, fn);
    if (rc) return rc;
    std::vector<std::vector<uint32_t>> parts(n);
    std::vector<const void *> ptrs(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        if (!plan.renders(i)) continue;
        parts[i].resize((size_t)plan.rows[i] * plan.width);
        const size_t part_bytes = parts[i].size() * sizeof(uint32_t);
        rc = which == 0 ? rtx_refine_counts_rows(g->m[i].ctx, parts[i].data(), part_bytes)
                        : rtx_refine_error_rows(g->m[i].ctx, reinterpret_cast<float *>(parts[i].data()), part_bytes);
        if (rc != RTX_OK) {
            const std::string why = rtx_last_error();
            return fail(rc, f + ": member " + std::to_string(i) + ": " + why);
        }
        ptrs[i] = parts[i].data();
    }
    rtx::group_gather_state(plan, ptrs.data(), host, sizeof(uint32_t));
    return RTX_OK;
}

}  // namespace

int rtx_group_refine_adaptive(rtx_group *g, uint32_t samples, float threshold, uint32_t max_samples,
                              uint32_t tile_rows, int reset, uint32_t *active) {
    // arguments and state first: nothing in this block touches HIP
    int rc = adaptive_call_check(g, "rtx_group_refine_adaptive", samples, threshold, max_samples, tile_rows);
    if (rc) return rc;
    const bool fresh = adaptive_fresh(g, tile_rows, reset);
    const uint32_t have = fresh ? 0u : g->ref_n;
    if (samples > 0xffffffffu - have)
        return fail(RTX_ERR_INVALID, "rtx_group_refine_adaptive: more than 2^32 - 1 samples in all");
    std::vector<uint32_t> act;
    rc = adaptive_phase1(g, "rtx_group_refine_adaptive", samples, threshold, max_samples, tile_rows, fresh, act);
    if (rc) return rc;
    uint64_t total = 0;
    for (uint32_t a : act) total += a;
    if (active) *active = (uint32_t)total;
    if (total == 0) return RTX_OK;  // nothing to trace: N, the image, the states and the maps stay
    rc = ensure_buffers(g, tile_rows);
    if (rc) return rc;
    const uint32_t n = (uint32_t)g->m.size();
    std::vector<uint32_t> member_n(n);
    for (uint32_t i = 0; i < n; ++i) member_n[i] = fresh ? 0u : g->m[i].ref_n;
    g->ref_n = 0;  // until every member's launch and the assembly are enqueued
    rc = run_frame(g, "rtx_group_refine_adaptive", [&](uint32_t i, uint32_t np, void *d_out) {
        Member &mb = g->m[i];
        // a member with rows but nothing to trace: its slot takes its rows as they are
        if (act[i] == 0) return rtx::ctx_state_image(mb.ctx, d_out);
        uint32_t got = 0;
        const int r = rtx_refine_adaptive_rows(mb.ctx, tile_rows, i, np, samples, threshold, max_samples, fresh ? 1 : 0,
                                               mb.d_halo, d_out, &got);
        if (r == RTX_OK && got != act[i])
            return fail(RTX_ERR_STATE, "its mask changed between the two phases (" + std::to_string(act[i]) + " then " +
                                           std::to_string(got) + " active pixels)");
        if (r == RTX_OK) member_n[i] += samples;
        return r;
    });
    if (rc != RTX_OK) return rc;
    g->ref_n = have + samples;
    g->ref_tile = tile_rows;
    for (uint32_t i = 0; i < n; ++i) g->m[i].ref_n = member_n[i];
    if (fresh) g->ref_mixed = false;
    if (total != (uint64_t)g->frame.width * g->frame.height) g->ref_mixed = true;
    return RTX_OK;
}

int rtx_group_refine_pending(rtx_group *g, uint32_t samples, float threshold, uint32_t max_samples, uint32_t tile_rows,
                             uint32_t *active) {
    int rc = adaptive_call_check(g, "rtx_group_refine_pending", samples, threshold, max_samples, tile_rows);
    if (rc) return rc;
    if (!active) return fail(RTX_ERR_INVALID, "rtx_group_refine_pending: null active");
    std::vector<uint32_t> act;
    rc = adaptive_phase1(g, "rtx_group_refine_pending", samples, threshold, max_samples, tile_rows,
                         adaptive_fresh(g, tile_rows, 0), act);
    if (rc) return rc;
    uint64_t total = 0;
    for (uint32_t a : act) total += a;
    *active = (uint32_t)total;
    return RTX_OK;
}

int rtx_group_refine_counts(rtx_group *g, uint32_t *host_counts, size_t bytes) {
    return group_read(g, "rtx_group_refine_counts", 0, host_counts, bytes);
}
int rtx_group_refine_error(rtx_group *g, float *host_err, size_t bytes) {
    return group_read(g, "rtx_group_refine_error", 1, host_err, bytes);
}

int rtx_group_get_accumulate_times(rtx_group *g, double *render_ms, double *gather_ms, double *fold_ms) {
    if (!g) return fail(RTX_ERR_INVALID, "rtx_group_get_accumulate_times: null group");
    if (!g->have_acc_times)
        return fail(RTX_ERR_STATE, "rtx_group_get_accumulate_times: no round synced (rtx_group_sync first)");
    if (render_ms)
        for (size_t i = 0; i < g->m.size(); ++i) render_ms[i] = g->acc_render_ms[i];
    if (gather_ms) *gather_ms = g->acc_gather_ms;
    if (fold_ms) *fold_ms = g->fold_ms;
    return RTX_OK;
}

int rtx_group_sync(rtx_group *g) {
    if (!g) return fail(RTX_ERR_INVALID, "rtx_group_sync: null group");
    int first = RTX_OK;
    std::string why;
    for (size_t i = 0; i < g->m.size(); ++i) {  // every member, also after a failure
        const int rc = rtx_sync(g->m[i].ctx);
        if (rc != RTX_OK && first == RTX_OK) {
            first = rc;
            why = "rtx_group_sync: member " + std::to_string(i) + ": " + rtx_last_error();
        }
    }
    if (first != RTX_OK) return fail(first, why);
    if (g->launched && !g->have_times) {
        float t = 0.0f;
        for (size_t i = 0; i < g->m.size(); ++i) {
            Member &mb = g->m[i];
            g->render_ms[i] = 0.0;
            if (!mb.rendered) continue;
            RTXG_HIP(hipSetDevice(mb.device));
            RTXG_HIP(hipEventElapsedTime(&t, mb.ev_start, mb.ev_rendered));
            g->render_ms[i] = t;
        }
        RTXG_HIP(hipSetDevice(g->m[0].device));
        RTXG_HIP(hipEventElapsedTime(&t, g->ev_g0, g->ev_g1));
        g->gather_ms = t;
        RTXG_HIP(hipEventElapsedTime(&t, g->ev_d0, g->ev_d1));
        g->deint_ms = t;
        g->have_times = true;
    }
    if (g->acc_launched && !g->have_acc_times) {  // the last round of the last rtx_group_accumulate
        float t = 0.0f;
        for (size_t i = 0; i < g->m.size(); ++i) {
            Member &mb = g->m[i];
            g->acc_render_ms[i] = 0.0;
            if (!mb.summed) continue;
            RTXG_HIP(hipSetDevice(mb.device));
            RTXG_HIP(hipEventElapsedTime(&t, mb.ev_sum0, mb.ev_sum1));
            g->acc_render_ms[i] = t;
        }
        RTXG_HIP(hipSetDevice(g->m[0].device));
        RTXG_HIP(hipEventElapsedTime(&t, g->ev_a0, g->ev_a1));
        g->acc_gather_ms = t;
        RTXG_HIP(hipEventElapsedTime(&t, g->ev_f0, g->ev_f1));
        g->fold_ms = t;
        g->have_acc_times = true;
    }
    return RTX_OK;
}

void *rtx_group_image(rtx_group *g) { return g ? g->d_image : nullptr; }

int rtx_group_download(rtx_group *g, float *host, size_t bytes) {
    if (!g || !host) return fail(RTX_ERR_INVALID, "rtx_group_download: null argument");
    if (!g->d_image || !(g->launched || g->acc_launched))
        return fail(RTX_ERR_STATE, "rtx_group_download: nothing rendered yet");
    if (bytes != g->image_pixels * rtx::kGroupPixelBytes)
        return fail(RTX_ERR_INVALID, "rtx_group_download: bytes != width*height*16");
    const int rc = rtx_group_sync(g);
    if (rc != RTX_OK) return rc;
    Member &root = g->m[0];
    RTXG_HIP(hipSetDevice(root.device));
    RTXG_HIP(hipMemcpyAsync(host, g->d_image, bytes, hipMemcpyDeviceToHost, root.stream));
    RTXG_HIP(hipStreamSynchronize(root.stream));
    return RTX_OK;
}

int rtx_group_get_times(rtx_group *g, double *render_ms, double *gather_ms, double *deinterleave_ms) {
    if (!g) return fail(RTX_ERR_INVALID, "rtx_group_get_times: null group");
    if (!g->have_times) return fail(RTX_ERR_STATE, "rtx_group_get_times: no frame synced (rtx_group_sync first)");
    if (render_ms)
        for (size_t i = 0; i < g->m.size(); ++i) render_ms[i] = g->render_ms[i];
    if (gather_ms) *gather_ms = g->gather_ms;
    if (deinterleave_ms) *deinterleave_ms = g->deint_ms;
    return RTX_OK;
}

}  // extern "C"
