// vk_api.hip — the C ABI of include/vecchio_amd.h (libvecchio_amd.so) around the HIP megakernel of vk_kernels.h.
//
// Kernel structure (gfx950 / CDNA4, wave64):
//   * persistent workgroups (256-1024 threads, sized by plan_residency; sphere-only scenes staged in LDS run as TWO concurrent
//     launches, one 1024-thread and one 768-thread workgroup per CU = seven waves per SIMD: launch_dual); each WAVE pulls work units =
//     (8x8-pixel tile, sample chunk) from a global atomic counter and hands them to its lanes sample by
//     sample; it pulls the next unit the moment the current one is handed out (no per-unit drain);
//   * one ray per lane.  A lane whose path ended takes the next (pixel, sample) through a ballot +
//     prefix-popcount ("active-ray compaction"); the RNG is keyed (seed, pixel, sample) and pixel sums are
//     64-bit fixed point (integer atomics: LDS per tile, flushed to the frame's accumulators once per
//     unit), so the image does not depend on which lane, wave, unit, tile partition or GPU traced a
//     sample, nor on completion order;
//   * a wave-level phase scheduler runs, each round, the code of the state most lanes are in: BOX
//     (box_steps: nested steps under one shrinking EXEC mask, light primitive tests inline), PRIM heavy,
//     SHADE + REFILL (out of line for the everything-variants); lane state that only shading needs
//     (throughput, RNG, depth, pixel) is parked in LDS between SHADE phases so the traversal loops fit
//     80 VGPRs (6 waves/SIMD; 72 = 7 for sphere-only scenes in LDS; 64 = 8 for sphere-only scenes traversed from global memory);
//   * traversal is the stack-free threaded walk of vk_trace.h; when the linear BVH + spheres + boxes
//     fit next to that per-wave state WITHOUT costing occupancy, every workgroup stages them into its
//     LDS (160 KB/CU) once and item fetches are ds_read_b128; otherwise they are L1/L2 gathers;
//   * scenes of spheres only are walked on a tree REBUILT over the reference's leaf units (vk_linearize.cpp), and the tree as handed
//     over decides every segment whose winner could depend on the visiting order (vk_trace.h segment_unsafe): walked again in place
//     where both trees sit in one array (global-memory scenes), or the sample is queued and rendered by a second launch of the same
//     kernel in list mode (LDS scenes: enqueue_render_f32);
//   * no MFMA: there is no dense contraction in a path tracer.
//
// Host side: one vk_scene per device (scene upload, per-launch scratch); vk_scene_create_multi = a group of
// them: tiles dealt over the devices, each on its own stream, slabs moved to devices[0] by peer copies,
// de-interleaved on device, one device-to-host copy.
//
// There is NO CPU fallback in this library: every entry point either runs on a gfx950
// device or returns an error.

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>      // declarations only: librccl.so is loaded on request (VK_SCENE_RCCL_GATHER), never linked

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vecchio_amd.h"
#include "../../include/vecchio_amd_debug.h"
#include "vk_linearize.h"
#include "vk_kernels.h"
#include "vk_adapt.h"        // the kernels of vk_adapt.hip: argument records and launchers
#include "vk_splat.h"        // the kernels of vk_splat.hip: the filter, argument records and launchers
#include "vk_robust.h"       // the kernels of vk_robust.hip: the per-pixel resolve, argument records and launchers
#include "vk_lpe.h"          // the kernels of vk_lpe.hip: the tag, the rule match, argument records and launchers
#include "vk_tone.h"         // the kernels of vk_tone.hip: the per-pixel display transform, argument records and launchers
#include "vk_nlm.h"          // the kernels of vk_nlm.hip: the non-local-means filter's per-pixel code, argument records and launchers
#include "vk_glare.h"        // the kernels of vk_glare.hip: the glare stage's per-pixel code, launch plan, argument records and launchers
#include "vk_psf.h"          // the kernels of vk_psf.hip: the point-spread stage's per-element code, tables, argument records and launchers
#include "vk_upsample.h"     // the kernels of vk_upsample.hip: guided upsampling's per-pixel code, argument records and launchers
#include "vk_matte.h"        // the kernels of vk_matte.hip: the table of a pixel, the argument record and launchers

namespace {

thread_local std::string g_err = "";

int fail(int code, const std::string &m) { g_err = m; return code; }

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return fail(VK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ---- RCCL, loaded on first use (VK_SCENE_RCCL_GATHER: the in-library gather of a multi-device scene as grouped ncclSend / ncclRecv).
// Not linked: a single-device host never maps librccl.so.
struct RcclApi {
    void *handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string why;
    bool ok() const { return handle && CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString; }
};
const RcclApi &rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
#ifdef VK_DEBUG_LIB
        // the DEBUG build may be pointed at a test double (tests/mock_rccl: the gather's orchestration on a one-GPU box)
        if (const char *e = getenv("VK_RCCL_LIB")) a.handle = dlopen(e, RTLD_NOW | RTLD_LOCAL);
#endif
        for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            if (a.handle) break;
            a.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        }
        if (!a.handle) { const char *e = dlerror(); a.why = std::string("librccl.so could not be loaded: ") + (e ? e : "?"); return a; }
#define VK_RCCL_SYM(field, sym) a.field = reinterpret_cast<decltype(a.field)>(dlsym(a.handle, #sym))
        VK_RCCL_SYM(CommInitAll, ncclCommInitAll); VK_RCCL_SYM(CommDestroy, ncclCommDestroy); VK_RCCL_SYM(GroupStart, ncclGroupStart);
        VK_RCCL_SYM(GroupEnd, ncclGroupEnd); VK_RCCL_SYM(Send, ncclSend); VK_RCCL_SYM(Recv, ncclRecv);
        VK_RCCL_SYM(GetErrorString, ncclGetErrorString);
#undef VK_RCCL_SYM
        if (!a.ok()) a.why = "librccl.so lacks one of ncclCommInitAll / ncclCommDestroy / ncclGroupStart / ncclGroupEnd / ncclSend / ncclRecv";
        return a;
    }();
    return api;
}
#define RCCL_TRY(expr)                                                                                                              \
    do {                                                                                                                            \
        ncclResult_t _r = (expr);                                                                                                   \
        if (_r != ncclSuccess) return fail(VK_ERR_HIP, std::string(#expr) + ": " + rccl_api().GetErrorString(_r));                  \
    } while (0)

// nothing may unwind across the C boundary: every entry point that can allocate runs through this
template <class Fn>
int guarded(Fn &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(VK_ERR_OOM, "out of host memory");
    } catch (const std::exception &e) {
        return fail(VK_ERR_BAD_ARG, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(VK_ERR_BAD_ARG, "internal error");
    }
}

// Diagnostic switches (environment), read ONCE per scene at creation: none changes a pixel (VK_CHUNK_CAP included: pixel sums are
// fixed-point integers, so their grouping into units does not matter; tests/test_gpu_launch_matrix.py checks every switch bit for bit).
// DESIGN.md §6 lists them.
struct EnvSwitches {
    bool force_full_variant = false;   // VK_FORCE_FULL_VARIANT=1: run the everything-kernel
    bool no_lds_scene = false;         // VK_NO_LDS_SCENE=1: traverse from global memory at full occupancy
    int max_waves_per_cu = 0;          // VK_MAX_WAVES_PER_CU=n: lower the occupancy
    int chunk_cap = 0;                 // VK_CHUNK_CAP=n: samples per pixel per work unit
    int shade_defer = 0;               // VK_SHADE_DEFER=n
    bool tile_order = true;            // VK_TILE_ORDER=0: raster order, no probe launch; =1: dearest-first also for whole frames
    bool tile_order_forced = false;
    int probe_spp = 0;                 // VK_PROBE_SPP=n
    int probe_depth = 0;               // VK_PROBE_DEPTH=n: depth limit of the probe launch's paths (default 16)
    int prim_weight = 0;               // VK_PRIM_WEIGHT=n
    bool order_reuse = true;           // VK_ORDER_REUSE=0: probe the tile costs in every frame of a partition
    bool dual_same_stream = false;     // VK_DUAL_SAME_STREAM=1 (tests): see launch_dual
    bool dual_debug = false;           // VK_DUAL_DEBUG=1: print each checked frame's unit split
    // VK_RETREE=0/1/2: nothing rebuilt / every draw-free subtree / exact re-treeing (default: vk_scene_desc.flags)
    int retree = -1;
    int redo_region_cap = 0;           // VK_REDO_REGION_CAP=n (tests): entries per queue between the two launches of exact re-treeing
    bool grid_global = false;          // VK_GRID_GLOBAL=1 (comparisons): the grid form also for scenes traversed from global memory
    bool no_grid = false;              // VK_NO_GRID=1 (comparisons): the tree forms of exact re-treeing where the grid form would do
    int near_lds = -1;                 // VK_NEAR_LDS=0/1 (comparisons): the near form of exact re-treeing from global memory / staged in LDS
    static int int_env(const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; }
    static EnvSwitches read() {
        EnvSwitches v;
        if (const char *e = getenv("VK_FORCE_FULL_VARIANT")) v.force_full_variant = e[0] == '1';
        if (const char *e = getenv("VK_NO_LDS_SCENE")) v.no_lds_scene = e[0] == '1';
        if (const char *e = getenv("VK_TILE_ORDER")) { v.tile_order = e[0] != '0'; v.tile_order_forced = e[0] == '1'; }
        if (const char *e = getenv("VK_RETREE")) v.retree = (e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
        if (const char *e = getenv("VK_DUAL_SAME_STREAM")) v.dual_same_stream = e[0] == '1';
        if (const char *e = getenv("VK_ORDER_REUSE")) v.order_reuse = e[0] != '0';
        if (const char *e = getenv("VK_DUAL_DEBUG")) v.dual_debug = e[0] == '1';
        v.max_waves_per_cu = int_env("VK_MAX_WAVES_PER_CU");
        v.chunk_cap = int_env("VK_CHUNK_CAP");
        v.shade_defer = int_env("VK_SHADE_DEFER");
        v.probe_spp = int_env("VK_PROBE_SPP");
        v.probe_depth = int_env("VK_PROBE_DEPTH");
        v.prim_weight = int_env("VK_PRIM_WEIGHT");
        v.redo_region_cap = int_env("VK_REDO_REGION_CAP");
        if (const char *e = getenv("VK_NEAR_LDS")) v.near_lds = e[0] != '0';
        if (const char *e = getenv("VK_NO_GRID")) v.no_grid = e[0] == '1';
        if (const char *e = getenv("VK_GRID_GLOBAL")) v.grid_global = e[0] == '1';
        return v;
    }
};

}  // namespace

#include "vk_resources.h"      // (uses fail() and HIP_TRY)
using vkr::DeviceBuffer;
using vkr::Event;
using vkr::PinnedBuffer;
using vkr::Stream;
static_assert(vkd::HANDED_OVER_T_MIN == T_MIN, "handed_over_view's tmin_gate is vk_trace.h's T_MIN");

// =========================================================================================
// One vk_scene = the linearised scene resident on ONE device plus the per-launch scratch of the (at most one)
// render in flight on it.  A multi-device scene (vk_scene_create_multi) is a group handle: `parts` holds one
// ordinary single-device scene per listed device, each with its own stream.
struct vk_scene {
    int device = 0;
    std::shared_ptr<const LinearScene> host;   // shared by the parts of a multi-device scene
    DScene dev;                // device pointers
    EnvSwitches env;
    std::vector<DeviceBuffer<>> allocs;        // the uploads `dev` (and rays.prov) point into
    DeviceBuffer<uint32_t> counter;
    DeviceBuffer<float> fb;                    // f32 framebuffer (vk_render; RGB8 output; the parts' render targets)
    DeviceBuffer<uint8_t> fb8;                 // RGB8 image for vk_render with VK_OUTPUT_RGB8
    DeviceBuffer<long long> accum;             // fixed-point pixel sums of the render in flight
    DeviceBuffer<float4> debug;
    Event ev0, ev1;
    int num_cus = 256;
    bool last_timed = false;
    DeviceBuffer<unsigned long long> wave_times;    // VK_WAVE_TIMES=1 (diagnostics)
    DeviceBuffer<unsigned long long> phase_stats;   // device, 24 counters (diagnostic kernel build)
    bool want_phase_stats = false;
    // the render_kernel launches of the last frame (vk_debug_last_launches: tests); host bookkeeping, cleared per frame
    std::vector<vk_debug_launch> launch_log;

    // ---- the residency plan (plan_residency)
    struct Residency {
        uint32_t lds_bytes = 0;    // hot-record bytes staged per workgroup (0 = not LDS resident)
        bool grid_on = false;      // the grid form of exact re-treeing is this scene's walk (DGrid)
        uint32_t grid_slots = 0;   // the grid form: size of the table [cells | refs] in 32-byte units (KArgs::lds_items of its launches)
        size_t hot_bytes = 0;      // items + spheres + boxes: what traversal gathers from
        uint32_t wg_threads = 512; // workgroup size chosen by plan_residency()
        uint32_t sphere_waves = 6; // waves per SIMD of the sphere-only variant (8 was measured 3 % slower: it spills)
        uint32_t wgs_per_cu = 2;
        // Seven waves per SIMD for sphere-only scenes staged in LDS: ONE 1024-thread and ONE 768-thread workgroup per CU, i.e. two
        // concurrent launches of the same kernel pulling from the same unit counter (plan_residency); the second one runs on
        // `dual.stream2`.
        bool dual_launch = false;
    } plan;

    // ---- the dual launch (launch_dual)
    struct Dual {
        Stream stream2;
        Event ev_fork, ev_join;
        // Self-check of the dual launch: the two launches must OVERLAP, or the first one does all the work at 16 waves per CU.  Each
        // launch counts the units it pulls (two words of the counter block); the 768-thread launch should get ~12/28 of them.  A frame
        // in which one launch got under a tenth counts as a strike; after two strikes in a row the scene uses the single-launch shape
        // for good.  Checked where the caller synchronises anyway (vk_scene_last_kernel_ms, vk_render).
        bool last = false;         // the last render used the dual launch
        int strikes = 0;
    } dual;

    // ---- exact re-treeing (vk_trace.h): the scene's own tree is a rebuilt one; samples it cannot vouch for are queued by the first
    // launch and rendered by a second one on `ref_view`, the scene as handed over.  redo_count: REDO_REGIONS counters + the 3 plan words.
    struct Exact {
        bool on = false;               // host->ref_items is there and the switch VK_EXACT_RETREE is not 0
        DScene ref_view;
        DeviceBuffer<uint2> redo_list;
        DeviceBuffer<uint32_t> redo_count;
        bool redo_last = false;        // the last render had a second launch
        // The rebuilt tree is SUSPENDED for a while when a frame sends more than a quarter of its samples through the second launch, or
        // overflows the queues between the launches (the fallback launch then renders the frame a third time): the scene renders on the
        // tree as handed over until frame `resume`, then tries again; every relapse doubles the pause (32 frames .. 4096).  An animation
        // that passes through one bad viewpoint loses the rebuilt tree for a few dozen frames, not for good.  The verdict on a frame is
        // read from `plan_host` (pinned; copied behind the frame's last kernel) when the NEXT frame is enqueued, without waiting, or
        // where the caller synchronises anyway (vk_scene_last_requeued_samples).
        uint64_t frame_no = 0, resume = 0, pause = 32;
        // Two verdict slots, used in turn: [4] words of a frame's redo_plan each, an event recorded right behind the copy, the samples
        // of the partition the frame covered.  A caller that always enqueues frame N + 1 before frame N has finished (vk_render_device
        // in a pipeline) still has frame N - 1's verdict taken when it enqueues frame N + 1: the verdict does not wait for the MOST
        // RECENT frame.
        PinnedBuffer<uint32_t> plan_host;  // [2][4]
        Event ev_plan[2];
        bool plan_pending[2] = {false, false};      // a frame with a second launch has been enqueued and its plan not judged yet
        uint64_t plan_samples[2] = {0, 0};
        int plan_last = 0;                 // the slot of the last frame with a second launch
        bool plan_copied = false;          // ... whose plan did travel to that slot
        uint64_t redo_last_samples = 0;    // samples of the partition the last render covered
    } exact;

    // ---- heavy-first tile order: per-tile times of the probe launch and the order derived from them
    struct TileOrder {
        DeviceBuffer<uint32_t> cost, order, hist;
        // Frame-to-frame reuse of the order: the frames of an animation (and the steps of a benchmark) see nearly the same tile costs,
        // so the order found for a partition is kept while the partition's geometry is the same, the camera has hardly moved and the
        // order is younger than ORDER_MAX_AGE frames; then the probe launch and the three sorting kernels are skipped (~1.7 ms of a
        // 1/8 share of C2's 42 ms).  The order never changes a pixel, so a stale one only costs balance.
        struct {
            uint32_t width = 0, height = 0, rank = 0, world = 0, depth = 0, age = 0;
            float org[3] = {0, 0, 0}, llc[3] = {0, 0, 0};
            bool valid = false;
        } made_for;
    } order;

    // ---- multi-device group (parts: empty for an ordinary scene)
    struct Group {
        std::vector<vk_scene *> parts;
        // a part's own stream, its slab (on its device), the slab's landing buffer on devices[0] and the event that says it landed
        Stream stream;
        DeviceBuffer<uint8_t> slab;
        DeviceBuffer<uint8_t> landing;
        Event ev_landed;
        Event ev_begin;                    // group: recorded on the caller's stream at the start of a frame
        // group, VK_SCENE_RCCL_GATHER: one communicator per part (rank j = devices[j]); empty = peer copies
        std::vector<ncclComm_t> comms;
    } group;

    // ---- vk_render_aov / vk_render_guides: their own events and output buffers, so that nothing that describes vk_render's last frame
    // is touched
    struct Aov {
        Event ev0, ev1;
        DeviceBuffer<float> buf;
    } aov;

    // ---- vk_render_mattes: its own events and staging buffer (ids, counts, overflow side by side), so that nothing of vk_render's last
    // frame or of vk_render_aov's results and times is touched
    struct Matte {
        Event ev0, ev1;
        DeviceBuffer<uint8_t> buf;
    } matte;

    // ---- vk_trace_rays: the provenance tables (uploaded by the scene's first ray query), the staging buffer of the host variant (rays,
    // then hits) and its events
    struct Rays {
        bool prov_ready = false;
        DProvenance prov = {nullptr, nullptr, nullptr, nullptr, nullptr};
        DeviceBuffer<uint8_t> buf;
        Event ev0, ev1;
    } rays;

    // ---- vk_denoise: the filter's scratch (two ping-pong images, the packed guides, the depth slopes), the device copies of
    // vk_denoise's host images, its own events (before the prepare kernel, behind it, behind every level), the levels of the last timed
    // call and the form the level kernels are launched in (vk_debug_denoise_form)
    struct Denoise {
        DeviceBuffer<uint8_t> buf;
        DeviceBuffer<float> io;
        Event ev[10];
        uint32_t last_levels = 0;
        int form = 0;
    } dn;
};

namespace {

// the scene that single-device work of a handle runs on: the scene itself, or devices[0]'s part of a multi-device group
vk_scene *first_part(vk_scene *s) { return s->group.parts.empty() ? s : s->group.parts[0]; }
const vk_scene *first_part(const vk_scene *s) { return s->group.parts.empty() ? s : s->group.parts[0]; }

template <class T>
int upload(vk_scene *s, const std::vector<T> &v, const T *&dptr) {
    dptr = nullptr;
    size_t bytes = v.size() * sizeof(T);
    s->allocs.emplace_back();
    DeviceBuffer<> &b = s->allocs.back();
    int rc = b.ensure(bytes);
    if (rc != VK_OK) return rc;
    if (bytes) HIP_TRY(hipMemcpy(b.get(), v.data(), bytes, hipMemcpyHostToDevice));
    dptr = reinterpret_cast<const T *>(b.get());
    return VK_OK;
}

constexpr uint32_t F_CORNELL = VKF_RECT | VKF_LIST | VKF_INSTANCE | VKF_BOX;

uint32_t pick_variant(const vk_scene *s) {
    const uint32_t features = s->host->features;
    if (s->env.force_full_variant) return VKF_ALL_SCENE;   // diagnostics: cost of the general kernel
    if (features == 0) return 0u;
    if ((features & ~F_CORNELL) == 0) return F_CORNELL;
    return VKF_ALL_SCENE;
}

// ---- the two choices of a kernel instance, each made in ONE place.  fn is a generic callable; it is handed the chosen feature set as a
// std::integral_constant<uint32_t, F> and what it returns is returned.
// The six variants of the path-tracing kernels (render_kernel, radiance_kernel, gather_kernel): F = pick_variant() | the integrator's bit.
template <class Fn>
auto with_variant(uint32_t F, Fn &&fn) {
    switch (F) {
        case 0u: return fn(std::integral_constant<uint32_t, 0u>{});
        case VKF_INTEG_PDF: return fn(std::integral_constant<uint32_t, (uint32_t)VKF_INTEG_PDF>{});
        case F_CORNELL: return fn(std::integral_constant<uint32_t, F_CORNELL>{});
        case F_CORNELL | VKF_INTEG_PDF: return fn(std::integral_constant<uint32_t, (F_CORNELL | VKF_INTEG_PDF)>{});
        case VKF_ALL_SCENE: return fn(std::integral_constant<uint32_t, (uint32_t)VKF_ALL_SCENE>{});
        default: return fn(std::integral_constant<uint32_t, (uint32_t)(VKF_ALL_SCENE | VKF_INTEG_PDF)>{});
    }
}
// The two instances of the single-walk kernels (first-hit buffers, guides, ray and occlusion queries): a sphere-only world takes the fused
// sphere path (C2), anything else the everything-variant.
template <class Fn>
auto with_walk_variant(uint32_t scene_features, Fn &&fn) {
    if (scene_features == 0u) return fn(std::integral_constant<uint32_t, 0u>{});
    return fn(std::integral_constant<uint32_t, (uint32_t)VKF_ALL_SCENE>{});
}

size_t per_wave_lds_bytes(uint32_t F) {   // cold lane state of one wave + its tile's fixed-point sums (64 x 3 x 8 B) + its unit state
    return ((F & VKF_INSTANCE) ? wave_block_floats<VKF_INSTANCE>() : wave_block_floats<0u>()) * sizeof(float);
}

// Waves per SIMD the variants with heavy primitives are built for (their __launch_bounds__): 80 VGPRs = 6, 96 = 5.
#ifndef VK_ALL_MINW
#define VK_ALL_MINW 6
#endif
#ifndef VK_CORNELL_MINW
#define VK_CORNELL_MINW 6
#endif
// LDS residency plan.  `hot` = bytes of items + spheres + boxes.  Measured on MI355X with the VALU-bound
// kernel: at EQUAL occupancy a scene staged in LDS beats the same scene read through L1/L2 by only 7 % (C2:
// 4.06 vs 3.77 Gsamples/s at 24 waves/CU; C4: no difference), while occupancy is worth much more (C3: the
// 118 KB scene in LDS leaves 11 waves/CU = 371 Msamples/s; from L2 at 16 waves/CU = 503).  So the scene is
// staged in LDS only when that costs no waves: choose the workgroup size (waves share one LDS copy) and
// workgroups per CU that reach the variant's full occupancy (24 waves/CU at 80 VGPRs) with the
// scene resident, else traverse from global memory at full occupancy.
void plan_residency(vk_scene *s, size_t hot) {
    const size_t pw = per_wave_lds_bytes(pick_variant(s));
    uint32_t best_waves = 0, best_wg = 0, best_n = 0;
    const bool spheres_only = pick_variant(s) == 0u;
    // The near form of exact re-treeing walks a failed segment again in place: both trees in items[], i.e. global memory — unless its
    // reach spans the small spheres' whole box: then hardly a segment fails (the InOneWeekend scene: 3 in 10^5), a failed one may as well
    // requeue its whole sample, and the scene is staged in LDS like any other (7 520 against the unit form's 7 285 Msamples/s at 256 spp)
    const bool near_needs_global = spheres_only && s->host->near_form && !s->plan.grid_on && (s->env.near_lds >= 0 ? s->env.near_lds == 0 : !s->host->near_spans);
    const uint32_t per_simd = spheres_only ? s->plan.sphere_waves : (pick_variant(s) == (uint32_t)VKF_ALL_SCENE ? (uint32_t)VK_ALL_MINW
                                                                                                           : (uint32_t)VK_CORNELL_MINW);   // = MINW of launch_variant
    uint32_t cap = 4 * per_simd;                                             // waves per CU the variant's register budget admits
    // Workgroups hold a multiple of 4 waves that divides evenly over the CU's four SIMDs: the dispatcher deals a workgroup's waves
    // round-robin, so e.g. two 10-wave workgroups land 3+3+2+2 twice and the second one does not fit beside the first at 5 per SIMD
    const uint32_t max_wg_waves = 12;                                        // <= the variants' __launch_bounds__ thread limit / 64
    { int v = s->env.max_waves_per_cu; if (v >= 4 && (uint32_t)v < cap) cap = (uint32_t)v; }   // diagnostics: lower the occupancy
    for (uint32_t n_wg = 1; n_wg <= 6; n_wg++) {
        size_t budget = LDS_PER_CU / n_wg;
        if (hot + 4 * pw > budget) break;
        uint32_t w = (uint32_t)std::min<size_t>(std::min<uint32_t>(max_wg_waves, cap / n_wg), (budget - hot) / pw);
        w &= ~3u;                          // (a multiple of four: see above)
        if (w < 4) break;
        if (w * n_wg > best_waves) { best_waves = w * n_wg; best_wg = w; best_n = n_wg; }
    }
    // Seven waves per SIMD (the sphere-only kernels need 72 VGPRs): 28 waves per CU cannot be two EQUAL workgroups — 14 waves land
    // 4+4+3+3 on the four SIMDs and the second workgroup does not fit beside the first — but they can be 16 + 12: a 1024-thread
    // workgroup (4 per SIMD) and a 768-thread one (3 per SIMD), from two concurrent launches.  Needs two LDS copies of the scene.
    s->plan.dual_launch = false;
    // (the near form of exact re-treeing walks a failed segment again in place: both trees in items[], i.e. global memory)
    if (spheres_only && !s->env.no_lds_scene && !near_needs_global && s->env.max_waves_per_cu == 0 && !getenv("VK_NO_DUAL_LAUNCH") &&
        2 * hot + 28 * pw <= LDS_PER_CU) {
        s->plan.lds_bytes = (uint32_t)hot; s->plan.wg_threads = 768; s->plan.wgs_per_cu = 2;      // (the single-launch shape: probe, STATS, tiny frames)
        s->plan.dual_launch = true;
        return;
    }
    if (best_waves >= cap && !s->env.no_lds_scene && !near_needs_global) {
        s->plan.lds_bytes = (uint32_t)hot; s->plan.wg_threads = best_wg * 64; s->plan.wgs_per_cu = best_n;
    } else {
        // 28 (sphere-only: seven 4-wave workgroups, 7 waves/SIMD) or 24 waves per CU
        s->plan.lds_bytes = 0; s->plan.wg_threads = 256; s->plan.wgs_per_cu = spheres_only ? 7 : per_simd;
    }
}

void log_launch(vk_scene *s, uint32_t role, uint32_t F, bool lds, int minw, bool cost, bool gridf, uint32_t grid, uint32_t block, size_t shmem) {
    vk_debug_launch r;
    r.role = role; r.features = F; r.lds_scene = lds; r.minw = (uint32_t)minw; r.cost = cost; r.grid_form = gridf;
    r.grid_size = grid; r.block_size = block; r.shmem_bytes = (uint32_t)shmem;
    s->launch_log.push_back(r);
}

template <uint32_t F, int MINW_SPHERES = 6>
int launch_variant(vk_scene *s, const KArgs &A, bool lds, dim3 grid, size_t shmem, hipStream_t st, bool cost) {
    // Register budget: every variant is held to 80 VGPRs = 6 waves per SIMD, 24 per CU.  The sphere-only kernels fit (76).  The
    // Cornell-type variants (Rect / list / Boxy / instance) need 96 and the everything-variants 120 to be free of spills, but both
    // gain more from the waves than they lose to the spills: C4 at 4 / 5 / 6 / 7 per SIMD 4 430 / 5 240 / 5 425 / 5 030 Msamples/s (45
    // spilled
    // registers at 6, 80 at 7, shading inline; out of line 5 340 at 6); C3, which waits for memory 44 % of the time, 642 / 695 / 726 at 4 /
    // 5 / 6
    // (13 spilled registers, 25 scratch instructions outside the box loop, shading out of line) and 695 at 7 (27 registers, 154).
    constexpr int MINW = ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) ? MINW_SPHERES
                                                                : ((F & VKF_ALL_SCENE) == VKF_ALL_SCENE ? VK_ALL_MINW : VK_CORNELL_MINW);
    // Sphere-only scenes traversed from GLOBAL memory (C5, 49 MB of items and spheres): every box step is a dependent gather there, so
    // waves in flight pay.  On the tree handed over 8 waves per SIMD / 64 VGPRs with the shading phase out of line were best (629 -> 685
    // Msamples/s over 6); on the rebuilt tree of exact re-treeing the walks are half as long and the 64-VGPR build's spills (72 B of
    // scratch per lane, 2 TB per frame) weigh more than the eighth wave: 6 / 7 / 8 waves per SIMD -> 1 112 / 1 163 / 1 076 Msamples/s.
    // Seven: 72 VGPRs, shading inline, seven 256-thread workgroups per CU.
    constexpr int MINW_G = ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) ? 7 : MINW;
    // Only the sphere-only kernels walk the rebuilt trees of exact re-treeing (segment_unsafe, the requeue, the redo walk in place) and only
    // F == 0 has a grid build: any other instance is handed the tree as handed over (create_on_device), never a rebuilt view
    if ((F & ~(uint32_t)VKF_INTEG_PDF) != 0u && (A.S.grid.nu != 0u || A.S.t_pad > 0.0f || A.S.walk_start != 0u))
        return fail(VK_ERR_BAD_ARG, "internal error: a view of a rebuilt tree for a kernel that cannot walk it");
    if (F != 0u && A.S.grid.nu != 0u) return fail(VK_ERR_BAD_ARG, "internal error: the grid form for a kernel without a grid build");
    const uint32_t role = cost ? VK_LAUNCH_PROBE : (A.list_mode == 1u ? VK_LAUNCH_REDO : (A.list_mode == 2u ? VK_LAUNCH_FALLBACK : VK_LAUNCH_MAIN));
    auto go = [&](auto kernel, bool l, int minw, bool gridf) -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(kernel, grid, dim3(s->plan.wg_threads), shmem, st, A);
        log_launch(s, role, F, l, minw, cost, gridf, grid.x, s->plan.wg_threads, shmem);
        return VK_OK;
    };
    int rc;
    if constexpr (F == 0u) {
        if (A.S.grid.nu != 0u) {      // the grid form of exact re-treeing (DGrid): worlds without lights, i.e. the scatter integrator's
            if (cost) rc = lds ? go(&render_kernel<F, true, MINW, false, true, true>, true, MINW, true)
                               : go(&render_kernel<F, false, MINW_G, false, true, true>, false, MINW_G, true);
            else rc = lds ? go(&render_kernel<F, true, MINW, false, false, true>, true, MINW, true)
                          : go(&render_kernel<F, false, MINW_G, false, false, true>, false, MINW_G, true);
            if (rc != VK_OK) return rc;
            HIP_TRY(hipGetLastError());
            return VK_OK;
        }
    }
    if (cost) rc = lds ? go(&render_kernel<F, true, MINW, false, true>, true, MINW, false) : go(&render_kernel<F, false, MINW_G, false, true>, false, MINW_G, false);
    else rc = lds ? go(&render_kernel<F, true, MINW, false, false>, true, MINW, false) : go(&render_kernel<F, false, MINW_G, false, false>, false, MINW_G, false);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

// The dual launch of plan_residency: the same 7-waves-per-SIMD build of a sphere-only LDS variant, once with 1024-thread workgroups on
// `st` and once with 768-thread workgroups on the scene's second stream, one workgroup of each per CU; both pull units from A.counter.
template <uint32_t F, bool GRID = false>
int launch_dual(vk_scene *s, const KArgs &A, size_t per_wave, hipStream_t st) {
    auto kernel = &render_kernel<F, true, 7, false, false, GRID>;
    const size_t shm_a = s->plan.lds_bytes + 16 * per_wave, shm_b = s->plan.lds_bytes + 12 * per_wave;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_a));
    // (VK_DUAL_SAME_STREAM=1, tests: both launches on ONE stream, i.e. serialised — what the self-check must notice)
    hipStream_t st2 = s->env.dual_same_stream ? st : s->dual.stream2;
    HIP_TRY(hipEventRecord(s->dual.ev_fork, st));                    // everything enqueued so far (memsets of counter and sums)
    HIP_TRY(hipStreamWaitEvent(st2, s->dual.ev_fork, 0));
    hipLaunchKernelGGL(kernel, dim3((unsigned)s->num_cus), dim3(1024), shm_a, st, A);
    hipLaunchKernelGGL(kernel, dim3((unsigned)s->num_cus), dim3(768), shm_b, st2, A);
    HIP_TRY(hipGetLastError());
    log_launch(s, VK_LAUNCH_DUAL_1024, F, true, 7, false, GRID, (uint32_t)s->num_cus, 1024u, shm_a);
    log_launch(s, VK_LAUNCH_DUAL_768, F, true, 7, false, GRID, (uint32_t)s->num_cus, 768u, shm_b);
    HIP_TRY(hipEventRecord(s->dual.ev_join, st2));
    HIP_TRY(hipStreamWaitEvent(st, s->dual.ev_join, 0));              // the resolve kernel waits for both
    s->dual.last = true;
    return VK_OK;
}

// cost = the probe build of the variant (per-tile times into A.tile_cost)
int launch_by_features(vk_scene *s, uint32_t F, const KArgs &A, bool lds, dim3 grid, size_t shmem, hipStream_t st, bool cost) {
    return with_variant(F, [&](auto f) { return launch_variant<decltype(f)::value>(s, A, lds, grid, shmem, st, cost); });
}

// what vk_render and the radiance queries refuse of a scene under an integrator
int check_integrator_for_scene(const LinearScene &H, uint32_t integrator) {
    if (integrator == VK_INTEGRATOR_PDF && H.lights.empty())
        return fail(VK_ERR_UNSUPPORTED, "PDF integrator with an empty lights list (Vec::random unwraps None, hittable.rs:431)");
    if (integrator == VK_INTEGRATOR_SCATTER && (H.features & VKF_SPEC_DIFFUSE))
        return fail(VK_ERR_UNSUPPORTED,
            "SpecDiffuse has no Material::scatter (default impl unwraps a None specular ray, material.rs:21-28)");
    return VK_OK;
}

// the checks of every call that takes a camera and render parameters (vk_render, vk_progress_create, vk_render_aov)
int check_call_args(vk_scene *scene, const vk_camera *cam, const vk_render_params *p) {
    if (!scene || !cam || !p) return fail(VK_ERR_BAD_ARG, "null argument");
    if (p->width < 2 || p->height < 2) return fail(VK_ERR_BAD_ARG,
        "width and height must be >= 2 (u,v divide by width-1/height-1, main.rs:187-188)");
    if ((uint64_t)p->width * p->height > (1ull << 31) / 3 || p->width > 65535u || p->height > 65535u) return fail(VK_ERR_BAD_ARG,
        "image too large");
    if (p->samples_per_pixel == 0 || p->samples_per_pixel > (1u << 26)) return fail(VK_ERR_BAD_ARG, "samples_per_pixel must be in 1..2^26");
    if (!(cam->time0 < cam->time1)) return fail(VK_ERR_BAD_ARG, "camera time0 >= time1 (gen_range panics, main.rs:118)");
    if (p->integrator > VK_INTEGRATOR_SCATTER || p->background > VK_BACKGROUND_SKY) return fail(VK_ERR_BAD_ARG,
        "bad integrator/background");
    if (p->output_format > VK_OUTPUT_RGB8) return fail(VK_ERR_BAD_ARG, "bad output_format");
    uint32_t world = p->tile_world ? p->tile_world : 1;
    if (p->tile_rank >= world) return fail(VK_ERR_BAD_ARG, "tile_rank >= tile_world");
    return VK_OK;
}

int check_render_args(vk_scene *scene, const vk_camera *cam, const vk_render_params *p) {
    int rc = check_call_args(scene, cam, p);
    if (rc != VK_OK) return rc;
    return check_integrator_for_scene(*scene->host, p->integrator);
}

struct TileGeom {      // the tile partition of one call
    uint32_t tiles_x, tiles_y, tiles, rank, world, n_local;
    TileGeom(const vk_render_params *p) {
        tiles_x = (p->width + TILE - 1) / TILE; tiles_y = (p->height + TILE - 1) / TILE; tiles = tiles_x * tiles_y;
        world = p->tile_world ? p->tile_world : 1; rank = p->tile_rank;
        n_local = tiles > rank ? (tiles - rank + world - 1) / world : 0;
    }
};

template <int MODE>
int tile_move(const void *src, void *dst, const vk_render_params *p, const TileGeom &g, hipStream_t st) {
    if (g.n_local == 0) return VK_OK;
    size_t n = (size_t)g.n_local * 64u;
    hipLaunchKernelGGL(tile_move_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, p->width, p->height,
        g.tiles_x,
                       g.rank, g.world, g.n_local);
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

uint64_t partition_samples(const vk_render_params *p, const TileGeom &g) {
    uint64_t px = 0;
    for (uint32_t t = g.rank; t < g.tiles; t += g.world) {
        uint32_t tx = (t % g.tiles_x) * TILE, ty = (t / g.tiles_x) * TILE;
        px += (uint64_t)std::min<uint32_t>(TILE, p->width - tx) * std::min<uint32_t>(TILE, p->height - ty);
    }
    return px * p->samples_per_pixel;
}

// number of sample chunks per tile.  Pixel sums are order independent, so this only sets the granularity of the work
// units (locality of a wave's samples against the spread of expensive tiles over many waves), never a pixel's value
// (active: the tiles an adaptive window renders, as far as the host knows — by default the partition's)
uint32_t choose_chunks(const vk_scene *s, const vk_render_params *p, const uint64_t *active = nullptr) {
    // Samples per pixel per unit: a unit keeps a wave on one tile (coherent primary rays, LDS tile sums flushed once per
    // unit); small enough that tiles of very different cost (fog, glass, grazing rays over 1M spheres) are spread over many
    // waves and that small images still give ~64K units for ~6K waves.  (C2: 32 / 64 / 128 spp per unit -> 5 218 / 5 235 / 5 221.)
    uint64_t tiles = (uint64_t)((p->width + TILE - 1) / TILE) * ((p->height + TILE - 1) / TILE);
    const uint64_t local = active ? *active : tiles / (p->tile_world ? p->tile_world : 1u);
    uint64_t c = (uint64_t)p->samples_per_pixel * local / 65536u;      // ~64K units per launch
    // One GPU: 64 (C2: 32 / 64 / 128 / 256 -> 5 218 / 5 235 / 5 221 / 4 960 Msamples/s).  One rank of N: the launch ends on the last
    // units of the rank's dearest tiles, so smaller ones (C2's 1/8 share: 64 -> 54.2 ms, 32 -> 53.1, 16 -> 52.9, 8 -> 53.5; ideal 50.0).
    // (seven waves per SIMD — the dual launch of sphere-only LDS scenes — like the smaller units too: 16 / 32 / 48 / 64 -> 6 805 / 6 836 /
    // 6 815 / 6 776 Msamples/s on C2 at full size)
    uint32_t cap = (p->tile_world > 1u || s->plan.dual_launch) ? 32u : 64u;
    // (Round 1 and the first half of round 2 cut the units of scenes bigger than an XCD's L2 down to 8 spp "because tile costs are
    // skewed by orders of magnitude": the skew was NaN rays walking the whole million-item tree — see begin_segment in vk_trace.h.
    // Without them C5 prefers the common setting: 4 / 8 / 16 / 32 / 64 spp per unit -> 564 / 574 / 579 / 583 / 585 Msamples/s.)
    if (s->env.chunk_cap >= 1) cap = (uint32_t)s->env.chunk_cap;   // diagnostics
    uint32_t lo = cap < 32 ? cap : 32;
    uint32_t chunk_spp = (uint32_t)(c > cap ? cap : (c < lo ? lo : c));
    // the unit counter is 32 bits wide: tiles x chunks must stay below 2^32 (4096 x 4096 at 2^20 spp would not at 64 spp per unit)
    {
        const uint64_t n_local = tiles / (p->tile_world ? p->tile_world : 1u) + 1u;
        const uint64_t min_chunk = ((uint64_t)p->samples_per_pixel * n_local + 0xE0000000ull - 1u) / 0xE0000000ull;
        if (chunk_spp < min_chunk) chunk_spp = (uint32_t)min_chunk;
    }
    uint32_t n = (p->samples_per_pixel + chunk_spp - 1) / chunk_spp;
    if (n < 1) n = 1;
    return n;
}

// The verdict on a frame with a second launch (its plan has arrived in slot b of plan_host): see vk_scene::Exact::resume.
void judge_frame(vk_scene *s, int b) {
    s->exact.plan_pending[b] = false;
    const uint32_t requeued = s->exact.plan_host[4 * b + 1], lost = s->exact.plan_host[4 * b + 2];
    const uint64_t frame_samples = s->exact.plan_samples[b];
    const bool heavy = (uint64_t)requeued * 4u > frame_samples && frame_samples >= (1u << 20);
    if (lost != 0u || heavy) {
        s->exact.resume = s->exact.frame_no + s->exact.pause;
        fprintf(stderr, "vecchio_amd: exact re-treeing %s (%u of %llu samples requeued, %u did not fit); this scene renders on the tree as "
            "handed over for the next %llu frames\n", lost ? "overflowed its queues and the frame was rendered again" : "sent over a quarter of "
            "a frame through the second launch", requeued, (unsigned long long)frame_samples, lost, (unsigned long long)s->exact.pause);
        s->exact.pause = std::min<uint64_t>(s->exact.pause * 2u, 4096u);
    } else if (s->exact.pause > 32u) {
        s->exact.pause /= 2u;           // a clean frame on the rebuilt tree: relapses are forgiven step by step
    }
}

// Progressive rendering (vk_progress_*): what one window of a handle asks of one device part.  p->samples_per_pixel is the WINDOW's
// length then (units, redo queues and the probe are sized by it); the clamp comes from the budget, so that clamping matches the one-shot
// frame of `budget` samples and `budget` samples can never overflow the running sums.
struct AccumDesc {
    uint32_t sample_base;          // the window's first sample
    uint32_t budget;               // the frame's total (vk_progress_info.samples_budget)
    uint32_t done;                 // samples in the running sums after this window
    long long *run;                // [width*height*3] running fixed-point sums, on the part's device
    double *m2;                    // [width*height*3] sum of n_j m_j^2 (VK_PROGRESS_STDERR), or null
    unsigned long long *clamped;   // running clamped-sample count
    hipEvent_t ev_done;            // recorded behind the window's accumulate kernel
    // adaptive windows (vk_progress_set_adaptive; tile_n == null: every tile of the partition is rendered), per local tile slot:
    uint32_t *tile_n, *tile_k;     // [n_local] samples / windows a converged tile froze with (0: active)
    uint32_t *list;                // [n_local] this window's active slots, in tile order (the compaction's output)
    uint32_t *ctl;                 // [0] their number (KArgs::active_count), [1] tiles left active after the judge, [2..3] their in-image
                                   // pixels (u64), [4..] the compaction's block counts
    uint32_t *h_left;              // pinned host copy of ctl[1..3], landed when ev_done has
    uint32_t steps;                // windows after this one
    uint32_t gate;                 // min_samples and min_steps are met after this window: tiles may converge
    float abs_tol, rel_tol;
    uint64_t known_tiles, known_px;   // active tiles and their in-image pixels as far as the host knows (sizing only, never a pixel)
};

// ---- enqueue_render_f32 and its stages, in the order it runs them.  Each stage enqueues on the call's stream `st` what its name says and
// hands what it decided to the later ones through its arguments.

// the verdicts that have arrived (never waits): the older slot first
void judge_arrived_frames(vk_scene *s) {
    for (int k = 1; k <= 2; k++) {
        const int b = (s->exact.plan_last + k) & 1;
        if (s->exact.plan_pending[b] && hipEventQuery(s->exact.ev_plan[b]) == hipSuccess) judge_frame(s, b);
    }
    (void)hipGetLastError();      // (hipErrorNotReady of a query is not an error of this call)
}

// Stage 1: takes the verdicts that have arrived; does this frame run on the rebuilt tree, with a second launch?
bool begin_frame_exact(vk_scene *s) {
    judge_arrived_frames(s);
    s->exact.frame_no++;
    return s->exact.on && !s->want_phase_stats && s->exact.frame_no >= s->exact.resume;     // (the diagnostic builds have no second launch)
}

// Stage 2, the near form: primary rays start on the tree as handed over when the camera (its lens included) is farther than `reach` from
// every sphere — their walk on the rebuilt tree could not stand (vk_trace.h begin_segment).  Decided from the box around the small spheres
// and the surfaces of the few big ones; when in doubt: no.  Writes view.primary_ref, or takes `exact` back.
void near_form_primary_rays(const vk_scene *s, const vk_camera *cam, DScene &view, bool &exact) {
    if (!(s->host->near_form && !s->plan.grid_on && (view.walk_start != 0u || s->exact.on) && s->host->n_big != 0xFFFFFFFFu)) return;
    const LinearScene &H = *s->host;
    const double reach = (double)H.reach + (double)fabsf(cam->lens_radius) * 1.5 + 1e-3 * (double)H.reach;
    double d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double o = cam->origin[k], e = o < H.small_lo[k] ? H.small_lo[k] - o : (o > H.small_hi[k] ? o - H.small_hi[k] : 0.0);
        d2 += e * e;
    }
    bool far_from_all = d2 > reach * reach;
    for (uint32_t b = 0; b < H.n_big && far_from_all; b++) {
        double q = 0.0;
        for (int k = 0; k < 3; k++) q += ((double)cam->origin[k] - H.big[b][k]) * ((double)cam->origin[k] - H.big[b][k]);
        far_from_all = fabs(sqrt(q) - (double)H.big[b][3]) > reach;
    }
    if (view.walk_start != 0u) view.primary_ref = far_from_all ? 1u : 0u;
    else if (far_from_all) exact = false;      // (staged in LDS there is one tree per launch: such a frame on the tree as handed over)
}

// Stage 3: the kernel's constants and everything of KArgs that does not depend on a later stage
int fill_render_args(vk_scene *s, const vk_camera *cam, const vk_render_params *p, const TileGeom &g, float *d_out, const AccumDesc *acc,
    hipStream_t st, KArgs &A) {
    A.C.cam = *cam;
    A.C.width = p->width; A.C.height = p->height; A.C.spp = p->samples_per_pixel; A.C.max_depth = p->max_depth;
    A.C.seed = p->seed; A.C.integrator = p->integrator; A.C.background = p->background;
    A.C.bg[0] = p->background_color[0]; A.C.bg[1] = p->background_color[1]; A.C.bg[2] = p->background_color[2];
    A.out = d_out;
    A.tiles_x = g.tiles_x; A.tiles_y = g.tiles_y;
    A.tile_rank = g.rank; A.tile_world = g.world;
    A.n_local_tiles = g.n_local;
    A.n_chunks = choose_chunks(s, p, acc && acc->tile_n ? &acc->known_tiles : nullptr);
#ifdef VK_WAVE_TIMES
    if (getenv("VK_WAVE_TIMES")) {
        int rc = s->wave_times.ensure(3u * 1024u * 16u * sizeof(unsigned long long));
        if (rc != VK_OK) return rc;
        HIP_TRY(hipMemsetAsync(s->wave_times, 0, 3u * 1024u * 16u * sizeof(unsigned long long), st));
        A.wave_times = s->wave_times;
    }
#else
    (void)st;
#endif
    A.counter = s->counter;
    A.clamped = reinterpret_cast<unsigned long long *>(s->counter.get()) + 1;     // bytes 8..15 of the counter block
    A.launch_units = s->counter + 4;                                         // bytes 16..23: units pulled by each launch of a dual launch
    A.accum_clamp = accum_clamp_for(acc ? acc->budget : p->samples_per_pixel);
    A.sample_base = acc ? acc->sample_base : 0u;
    A.shade_defer = SHADE_DEFER;          // (C5: 1 / 2 / 4 / 8 -> 573 / 588 / 593 / 603-at-pw-2)
    if (s->env.shade_defer >= 1 && s->env.shade_defer <= 64) A.shade_defer = (uint32_t)s->env.shade_defer;   // diagnostics
    // scenes beyond an XCD's L2 (C5: a leaf every 6 box steps, every gather a possible L2 miss): pending sphere tests are served
    // sooner — when 3x their lanes outnumber the stepping ones (1 / 2 / 3 -> 606 / 623 / 631 Msamples/s); L2-resident scenes: 1
    A.prim_weight = s->plan.hot_bytes > (4u << 20) ? 3u : 1u;
    if (s->env.prim_weight >= 1 && s->env.prim_weight <= 64) A.prim_weight = (uint32_t)s->env.prim_weight;   // diagnostics
    return VK_OK;
}

// Stage 4, max_depth == 0: ray_color returns (0,0,0) before tracing anything when depth (1) > MAX_DEPTH (main.rs:126-128): a black
// partition, nothing launched
int enqueue_black_frame(vk_scene *s, const vk_render_params *p, const TileGeom &g, float *d_out, hipStream_t st, const AccumDesc *acc) {
    HIP_TRY(hipMemsetAsync(s->counter, 0, 32, st));
    int rc = tile_move<TM_ZERO_F32>(nullptr, d_out, p, g, st);
    if (rc != VK_OK) return rc;
    if (acc) HIP_TRY(hipEventRecord(acc->ev_done, st));     // (every sample is (0,0,0): the running sums stay 0, so does their mean)
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->last_timed = true;
    s->exact.redo_last = false; s->dual.last = false;      // (nothing was launched: no second launch, no unit split to judge)
    return VK_OK;
}

// Heavy-first tile order.  A launch ends when its slowest unit does, and tile costs are skewed (C2's glass tiles cost 8x
// the mean, units that start mid-launch finish last).  So a probe launch of a few samples per pixel times every tile
// (the COST build of the same kernel variant), three tiny kernels bucket-sort the tiles dearest first, and the real
// launch takes its units in that order (longest processing time first).  The order never changes a pixel.
// One rank's 1/8 share of C2: 78.1 -> 68.6 ms (ideal 64.9); whole frame 522 -> 519 ms including the probe.
// (whole frames on one GPU gain nothing from it any more — there is no per-unit drain — and the 1 M-sphere scene loses 12 %
// with its dearest tiles all in flight at once; one rank's 1/8 share of C2: 59.7 ms in raster order, 53.9 dearest first, ideal 50.0)
// Does this frame take its tiles in that order?  If so, the order's buffers are there afterwards.
int want_tile_order(vk_scene *s, const vk_render_params *p, const TileGeom &g, bool &use_order) {
    use_order = g.n_local >= 64 && p->samples_per_pixel >= 64 && s->env.tile_order && (g.world > 1u || s->env.tile_order_forced);
    if (!use_order) return VK_OK;
    int rc = s->order.cost.ensure((size_t)g.tiles * sizeof(uint32_t));
    if (rc == VK_OK) rc = s->order.order.ensure((size_t)g.n_local * sizeof(uint32_t));
    if (rc == VK_OK) rc = s->order.hist.ensure(ORDER_BUCKETS * sizeof(uint32_t));
    return rc;
}

// Stage 5: sizes and arms the queues between the two launches of exact re-treeing; takes `exact` back when there is no memory for
// them.  Without a second launch the frame's view is the tree as handed over.
int arm_redo_queues(vk_scene *s, uint64_t frame_samples, hipStream_t st, KArgs &A, bool &exact) {
    uint64_t per_region = 0;
    if (exact) {
        // queues for the samples the first launch drops: room for 1/32 of the partition's samples (C2 drops 0.05 %; 8 bytes each: 0.5 GB
        // for C2's 2.1 G samples), spread over REDO_REGIONS; a full queue is reported where the caller synchronises
        // (vk_scene_last_requeued_samples), vk_render then renders the frame again on the tree as handed over
        // (at most 256 MB: a frame that needs more overflows, and the fallback launch renders it on the tree as handed over)
        // (an adaptive window: the samples of its active tiles, the tree's verdict judges what was rendered)
        s->exact.redo_last_samples = frame_samples;
        per_region = std::min<uint64_t>(frame_samples / 32u / REDO_REGIONS + 4096u, (256ull << 20) / sizeof(uint2) / REDO_REGIONS);
        // (the grid form seen from far away — the 1 M-sphere scene's camera — requeues 4 % of its samples: hits reported before the ray
        // enters their leaf's box, see segment_unsafe; room for an eighth, up to 4 GB of the 288)
        if (s->plan.grid_on && s->plan.lds_bytes == 0) per_region = std::min<uint64_t>(frame_samples / 8u / REDO_REGIONS + 4096u, (4096ull << 20) / sizeof(uint2) / REDO_REGIONS);
        if (s->env.redo_region_cap >= 1) per_region = (uint64_t)s->env.redo_region_cap;      // tests
        // (no memory for the queues: this frame on the tree as handed over, which needs none)
        if (s->exact.redo_list.ensure((size_t)per_region * REDO_REGIONS * sizeof(uint2)) != VK_OK) { (void)hipGetLastError(); exact = false; }
    }
    if (exact) {
        HIP_TRY(hipMemsetAsync(s->exact.redo_count, 0, (REDO_REGIONS * REDO_COUNT_STRIDE + 16) * sizeof(uint32_t), st));
        A.redo_list = s->exact.redo_list; A.redo_count = s->exact.redo_count; A.redo_plan = s->exact.redo_count + REDO_REGIONS * REDO_COUNT_STRIDE;
        A.redo_region_cap = (uint32_t)per_region;
    } else if (s->exact.on) {
        A.S = s->exact.ref_view;      // no second launch (diagnostic builds, a scene switched off, an oversized frame): the tree as handed over
    }
    // (the diagnostic builds have no grid walk: the tree as handed over, which is what items[] holds for a grid scene in global memory)
    if (s->plan.grid_on && s->want_phase_stats && A.S.grid.nu != 0u) A.S = handed_over_view(A.S);
    return VK_OK;
}

// the shape of a frame's launches: LDS residency of the hot records, the persistent grid, the kernel variant
struct LaunchShape {
    bool lds; uint32_t waves_per_wg; size_t shmem;
    uint64_t n_units;      // units the main launch will find, as far as the host knows
    uint32_t grid;         // enough workgroups to fill the chip, never more than there are units
    uint32_t F;
};

int plan_launch(const vk_scene *s, const vk_render_params *p, const AccumDesc *acc, KArgs &A, LaunchShape &L) {
    L.lds = s->plan.lds_bytes != 0;
    L.waves_per_wg = s->plan.wg_threads / 64;
    L.shmem = (size_t)L.waves_per_wg * per_wave_lds_bytes(pick_variant(s));
    if (L.lds) { A.lds_items = A.S.grid.nu != 0u ? s->plan.grid_slots : A.S.n_items; A.lds_spheres = s->dev.n_spheres; A.lds_boxes = s->dev.n_boxes;
        L.shmem += s->plan.lds_bytes; }
    // (choose_chunks keeps it below)
    if ((uint64_t)A.n_local_tiles * A.n_chunks >= 0xFFFFFFFFull) return fail(VK_ERR_BAD_ARG, "tiles x sample chunks exceeds the 32-bit unit counter");
    // the grid and the dual launch are sized from the units an adaptive window will find, as far as the host knows
    L.n_units = (acc && acc->tile_n ? acc->known_tiles : (uint64_t)A.n_local_tiles) * A.n_chunks;
    L.grid = (uint32_t)s->num_cus * s->plan.wgs_per_cu;
    uint64_t need_wgs = (L.n_units + L.waves_per_wg - 1) / L.waves_per_wg;
    if (L.grid > need_wgs) L.grid = (uint32_t)need_wgs;
    if (L.grid < 1) L.grid = 1;
    L.F = pick_variant(s) | (p->integrator == VK_INTEGRATOR_PDF ? (uint32_t)VKF_INTEG_PDF : 0u);
    return VK_OK;
}

// Stage 6: the order of want_tile_order into A.tile_order — the one kept from an earlier frame of this partition, or a probe launch and
// the three sorting kernels
int enqueue_tile_order(vk_scene *s, const vk_camera *cam, const vk_render_params *p, const TileGeom &g, const LaunchShape &L, hipStream_t st,
    KArgs &A) {
    auto &o = s->order.made_for;
    if (s->env.order_reuse) {      // (VK_ORDER_REUSE=0 probes every frame)
        auto close3 = [](const float *a, const float *b, float scale) {
            float d = fabsf(a[0] - b[0]) + fabsf(a[1] - b[1]) + fabsf(a[2] - b[2]);
            return d <= 0.05f * scale;
        };
        const float hscale = fabsf(cam->horizontal[0]) + fabsf(cam->horizontal[1]) + fabsf(cam->horizontal[2]) +
                             fabsf(cam->vertical[0]) + fabsf(cam->vertical[1]) + fabsf(cam->vertical[2]);      // size of the view plane
        const bool reuse = o.valid && o.width == p->width && o.height == p->height && o.rank == g.rank && o.world == g.world &&
                           o.depth == p->max_depth && o.age < 16u && close3(o.org, cam->origin, hscale) &&
                           close3(o.llc, cam->lower_left_corner, hscale);
        if (reuse) { o.age++; A.tile_order = s->order.order; return VK_OK; }
    }
    KArgs B = A;                                   // the probe: the same view at 1..4 samples per pixel, one unit per tile
    // (C2, one rank's 1/8 share: probe of 1 / 2 / 4 / 8 / 16 spp -> 68.6 / 69.0 / 69.8 / 70.5 / 73.0 ms: more samples cost more than
    // they sort better)
    B.C.spp = p->samples_per_pixel / 1024u; B.C.spp = B.C.spp < 1u ? 1u : (B.C.spp > 4u ? 4u : B.C.spp);
    // diagnostics
    if (s->env.probe_spp >= 1 && (uint32_t)s->env.probe_spp <= p->samples_per_pixel) B.C.spp = (uint32_t)s->env.probe_spp;
    // the probe only ranks the tiles: its paths are cut at 16 segments, so that this short launch does not end on a handful of
    // 50-segment paths (one rank's 1/8 share, efficiency against the whole frame / 8 with the cut at 50 / 16 / 8: C2 0.937 / 0.949 /
    // 0.948, C3 0.93 / 0.95 / 0.96, C5 0.957 / 0.957 / 0.951 — deep paths are part of what makes C5's tiles dear)
    {
        const uint32_t cut = s->env.probe_depth >= 1 ? (uint32_t)s->env.probe_depth : 16u;
        if (B.C.max_depth > cut) B.C.max_depth = cut;
    }
    B.n_chunks = 1; B.accum = nullptr; B.debug = nullptr; B.tile_order = nullptr;   // no sums: the probe only times the tiles
    B.redo_list = nullptr;                         // ... and drops nothing
    B.tile_cost = s->order.cost;
    HIP_TRY(hipMemsetAsync(s->order.cost, 0, (size_t)g.tiles * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(s->counter, 0, sizeof(uint32_t), st));
    uint32_t pgrid = (uint32_t)s->num_cus * s->plan.wgs_per_cu, pneed = (A.n_local_tiles + L.waves_per_wg - 1) / L.waves_per_wg;
    if (pgrid > pneed) pgrid = pneed;
    int rc = launch_by_features(s, L.F, B, L.lds, dim3(pgrid), L.shmem, st, true);
    if (rc != VK_OK) return rc;
    uint32_t nb = (A.n_local_tiles + 255u) / 256u;
    HIP_TRY(hipMemsetAsync(s->order.hist, 0, ORDER_BUCKETS * sizeof(uint32_t), st));
    hipLaunchKernelGGL(order_hist_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)s->order.cost, A.n_local_tiles, A.tile_rank,
        A.tile_world, s->order.hist.get());
    hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(1), 0, st, s->order.hist.get());
    hipLaunchKernelGGL(order_scatter_kernel, dim3(nb), dim3(256), 0, st, s->order.cost.get(), A.n_local_tiles, A.tile_rank, A.tile_world,
        s->order.hist.get(), s->order.order.get());
    HIP_TRY(hipGetLastError());
    A.tile_order = s->order.order;
    o.valid = true; o.width = p->width; o.height = p->height; o.rank = g.rank; o.world = g.world; o.depth = p->max_depth; o.age = 0;
    for (int k = 0; k < 3; k++) { o.org[k] = cam->origin[k]; o.llc[k] = cam->lower_left_corner[k]; }
    return VK_OK;
}

// Stage 7, an adaptive window: the active slots, filtered from the tile order of this window (dearest first, or raster): count, then
// scatter in order
int enqueue_adaptive_compaction(const AccumDesc *acc, const TileGeom &g, hipStream_t st, KArgs &A) {
    if (g.n_local == 0) {
        HIP_TRY(hipMemsetAsync(acc->ctl, 0, sizeof(uint32_t), st));
    } else {
        const uint32_t nb = (g.n_local + 1023u) / 1024u;
        hipLaunchKernelGGL(adaptive_count_kernel, dim3(nb), dim3(1024), 0, st, A.tile_order, (const uint32_t *)acc->tile_n, g.n_local,
                           acc->ctl + 4);
        hipLaunchKernelGGL(adaptive_scatter_kernel, dim3(nb), dim3(1024), 0, st, A.tile_order, (const uint32_t *)acc->tile_n, g.n_local,
                           (const uint32_t *)(acc->ctl + 4), acc->list, acc->ctl);
        HIP_TRY(hipGetLastError());
    }
    A.tile_order = acc->list;
    A.active_count = acc->ctl;
    return VK_OK;
}

#ifdef VK_DEBUG_LIB
// Stage 8 of vk_debug_phase_stats: the instrumented (STATS) build of the variant, in the single-launch shape
int launch_phase_stats(vk_scene *s, const LaunchShape &L, hipStream_t st, KArgs &A) {
    const uint32_t FULLPDF = VKF_ALL_SCENE | VKF_INTEG_PDF;
    const uint32_t CORNELLPDF = VKF_RECT | VKF_LIST | VKF_INSTANCE | VKF_BOX | VKF_INTEG_PDF;
    if (L.F != 0u && L.F != FULLPDF && L.F != CORNELLPDF)
        return fail(VK_ERR_UNSUPPORTED, "phase statistics are only built for the sphere-only/scatter, the Cornell-type/PDF and the full/PDF variants");
    int rc = s->phase_stats.ensure(24 * sizeof(unsigned long long));
    if (rc != VK_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->phase_stats, 0, 24 * sizeof(unsigned long long), st));
    A.phase_stats = s->phase_stats;
    auto go = [&](auto kernel) -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.shmem));
        hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(s->plan.wg_threads), L.shmem, st, A);
        return VK_OK;
    };
    if (L.F == 0u) rc = L.lds ? go(&render_kernel<0u, true, 6, true>) : go(&render_kernel<0u, false, 6, true>);
    else if (L.F == CORNELLPDF) rc = L.lds ? go(&render_kernel<CORNELLPDF, true, 6, true>) : go(&render_kernel<CORNELLPDF, false, 6, true>);
    else rc = L.lds ? go(&render_kernel<FULLPDF, true, 4, true>) : go(&render_kernel<FULLPDF, false, 4, true>);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipGetLastError());
    return VK_OK;
}
#endif

// Stage 8: the frame's launch — with enough units for 28 waves per CU to stay busy the dual launch, else (tiny frames) the single
// 2 x 768-thread shape
int launch_main(vk_scene *s, const LaunchShape &L, hipStream_t st, KArgs &A) {
    const bool dual = s->plan.dual_launch && L.lds && L.n_units >= (uint64_t)s->num_cus * 28u * 4u && s->dual.stream2;
    if (dual) {
        // seven waves per SIMD hide more of a parked lane's wait: shading deferred 5x, pending sphere tests served at 2x weight
        // (C2 at 256 spp, (defer, weight): (4,1) 6 098, (5,1) 6 166, (5,2) 6 230, (6,2) 6 208, (8,2) 6 230, (5,3) 6 071 Msamples/s)
        // (on the rebuilt tree of exact re-treeing, 256 spp: (4,1) 7 295, (5,2) 7 395, (6,2) 7 445, (8,2) 7 435, (6,3) 7 444)
        if (!(s->env.shade_defer >= 1 && s->env.shade_defer <= 64)) A.shade_defer = 6u;
        if (!(s->env.prim_weight >= 1 && s->env.prim_weight <= 64)) A.prim_weight = 2u;
    }
    const bool gridw = A.S.grid.nu != 0u;
    if (dual && L.F == 0u) return gridw ? launch_dual<0u, true>(s, A, per_wave_lds_bytes(0u), st) : launch_dual<0u>(s, A, per_wave_lds_bytes(0u), st);
    if (dual && L.F == (uint32_t)VKF_INTEG_PDF) return launch_dual<VKF_INTEG_PDF>(s, A, per_wave_lds_bytes(0u), st);
    return launch_by_features(s, L.F, A, L.lds, dim3(L.grid), L.shmem, st, false);
}

// Stage 9, exact re-treeing: the second launch, the fallback launch behind it and the copy of the frame's plan to a verdict slot
int enqueue_redo(vk_scene *s, const KArgs &A, const LaunchShape &L, size_t n_pixels, hipStream_t st) {
    // the second launch: the queued samples on the scene as handed over, in the single-launch shape
    uint32_t *plan = s->exact.redo_count + REDO_REGIONS * REDO_COUNT_STRIDE;
    hipLaunchKernelGGL(redo_plan_kernel, dim3(1), dim3(REDO_REGIONS), 0, st, (const uint32_t *)s->exact.redo_count, A.redo_region_cap, plan,
        (uint32_t)s->num_cus * s->plan.wgs_per_cu * L.waves_per_wg);
    HIP_TRY(hipMemsetAsync(s->counter, 0, sizeof(uint32_t), st));      // the unit counter only: clamped samples and unit counts add up
    KArgs B = A;
    B.S = s->exact.ref_view; B.list_mode = 1u; B.tile_order = nullptr; B.active_count = nullptr; B.wave_times = nullptr;
    if (L.lds) B.lds_items = B.S.n_items;
    B.shade_defer = SHADE_DEFER; B.prim_weight = s->plan.hot_bytes > (4u << 20) ? 3u : 1u;
    int rc = launch_by_features(s, L.F, B, L.lds, dim3((uint32_t)s->num_cus * s->plan.wgs_per_cu), L.shmem, st, false);
    if (rc != VK_OK) return rc;
    // ... and the fallback behind it: should a queue have overflowed, the sums are cleared and the partition is rendered on the tree
    // as handed over, so that a frame is never incomplete whoever the caller is (nearly always: two launches that return at once)
    hipLaunchKernelGGL(redo_reset_kernel, dim3(1024), dim3(256), 0, st, (const uint32_t *)plan, reinterpret_cast<unsigned long long *>(s->accum.get()),
        n_pixels * 3, s->counter.get());
    KArgs Fb = A;
    Fb.S = s->exact.ref_view; Fb.list_mode = 2u; Fb.redo_list = nullptr; Fb.wave_times = nullptr;
    if (L.lds) Fb.lds_items = Fb.S.n_items;
    Fb.shade_defer = SHADE_DEFER; Fb.prim_weight = B.prim_weight;
    rc = launch_by_features(s, L.F, Fb, L.lds, dim3(L.grid), L.shmem, st, false);
    if (rc != VK_OK) return rc;
    // the plan travels to the slot the previous frame did not use — unless that slot's verdict is still in flight (two frames behind and
    // not finished: the caller runs far ahead), then this frame goes unjudged rather than overwriting it
    const int b = s->exact.plan_last ^ 1;
    s->exact.redo_last = true;
    if (!s->exact.plan_pending[b]) {
        HIP_TRY(hipMemcpyAsync(s->exact.plan_host + 4 * b, plan, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(s->exact.ev_plan[b], st));
        s->exact.plan_pending[b] = true; s->exact.plan_samples[b] = s->exact.redo_last_samples; s->exact.plan_last = b;
        s->exact.plan_copied = true;
    } else s->exact.plan_copied = false;
    return VK_OK;
}

// Stage 10: the frame's fixed-point sums into d_out — plainly, into a progressive handle's running sums, or as an adaptive window
int enqueue_resolve(const KArgs &A, const vk_render_params *p, const TileGeom &g, float *d_out, const AccumDesc *acc, hipStream_t st) {
    const size_t n_pixels = (size_t)p->width * p->height;
    const uint32_t blocks = (uint32_t)((n_pixels + 255) / 256);
    if (acc && acc->tile_n) {
        // adaptive: the active tiles' sums into the running sums, every pixel's mean over its tile's samples into d_out; then the judge
        // freezes the tiles that have converged and counts the others for the host (pinned copy, landed by ev_done)
        hipLaunchKernelGGL(adaptive_resolve_kernel, dim3(blocks), dim3(256), 0, st, (const long long *)A.accum, acc->run, acc->m2, d_out,
                           p->width, p->height, p->samples_per_pixel, acc->done, A.tiles_x, A.tile_rank, A.tile_world,
                           (const uint32_t *)acc->tile_n, (const unsigned long long *)A.clamped, acc->clamped);
        HIP_TRY(hipMemsetAsync(acc->ctl + 1, 0, 3 * sizeof(uint32_t), st));
        if (g.n_local != 0)
            hipLaunchKernelGGL(adaptive_judge_kernel, dim3((g.n_local + 3u) / 4u), dim3(256), 0, st, (const long long *)acc->run,
                               (const double *)acc->m2, p->width, p->height, A.tiles_x, A.tile_rank, A.tile_world, g.n_local, acc->done,
                               acc->steps, acc->gate, acc->abs_tol, acc->rel_tol, acc->tile_n, acc->tile_k, acc->ctl + 1,
                               reinterpret_cast<unsigned long long *>(acc->ctl + 2));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(acc->h_left, acc->ctl + 1, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(acc->ev_done, st));
    } else if (acc) {
        // progressive: the window's sums into the running sums, the running mean into d_out (the window's sums stay in s->accum until
        // here, so the fallback launch re-renders this window only and earlier windows are untouched)
        hipLaunchKernelGGL(accumulate_resolve_kernel, dim3(blocks), dim3(256), 0, st, (const long long *)A.accum, acc->run, acc->m2, d_out,
                           p->width, p->height, p->samples_per_pixel, acc->done, A.tiles_x, A.tile_rank, A.tile_world,
                           (const unsigned long long *)A.clamped, acc->clamped);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(acc->ev_done, st));
    } else {
        hipLaunchKernelGGL(resolve_kernel, dim3(blocks), dim3(256), 0, st, (const long long *)A.accum, d_out, p->width, p->height,
                           p->samples_per_pixel, A.tiles_x, A.tile_rank, A.tile_world);
        HIP_TRY(hipGetLastError());
    }
    return VK_OK;
}

// Enqueues one render of this call's tile partition into the f32 framebuffer d_out (device memory of s->device) on `st`.  With `acc`
// (progressive rendering): one window of samples, added into acc's running sums, d_out = their running mean.
int enqueue_render_f32(vk_scene *s, const vk_camera *cam, const vk_render_params *p, float *d_out, hipStream_t st, bool want_debug,
    vk_stats *stats, const AccumDesc *acc = nullptr) {
    HIP_TRY(hipSetDevice(s->device));
    s->launch_log.clear();
    const TileGeom g(p);
    const bool adapt = acc && acc->tile_n;
    const size_t n_pixels = (size_t)p->width * p->height;
    // (an adaptive window: the samples of its active tiles, as far as the host knows)
    const uint64_t frame_samples = adapt ? acc->known_px * p->samples_per_pixel : partition_samples(p, g);
    KArgs A;
    memset(&A, 0, sizeof(A));
    A.S = s->dev;
    bool exact = begin_frame_exact(s);
    near_form_primary_rays(s, cam, A.S, exact);
    int rc = fill_render_args(s, cam, p, g, d_out, acc, st, A);
    if (rc != VK_OK) return rc;
    if (stats) {
        stats->samples = frame_samples;
        stats->kernel_launches = p->max_depth == 0 ? 1 : 2;      // (render + resolve)
        stats->scene_in_lds = s->plan.lds_bytes ? 1u : 0u;
        stats->kernel_ms = 0.0; stats->seconds = 0.0;
    }
    if (want_debug) {
        size_t need = n_pixels * p->samples_per_pixel * sizeof(float4);
        rc = s->debug.ensure(need);
        if (rc != VK_OK) return rc;
        HIP_TRY(hipMemsetAsync(s->debug, 0, need, st));
        A.debug = s->debug;
    }
    HIP_TRY(hipEventRecord(s->ev0, st));
    if (p->max_depth == 0) return enqueue_black_frame(s, p, g, d_out, st, acc);
    bool use_order = false;
    rc = want_tile_order(s, p, g, use_order);
    if (rc != VK_OK) return rc;
    {   // order-independent pixel sums (vk_kernels.h to_fixed): zeroed per frame, resolved into d_out after the launch
        rc = s->accum.ensure(n_pixels * 3 * sizeof(long long));
        if (rc != VK_OK) return rc;
        HIP_TRY(hipMemsetAsync(s->accum, 0, n_pixels * 3 * sizeof(long long), st));
        A.accum = s->accum;
    }
    s->exact.redo_last = false;
    s->dual.last = false;
    rc = arm_redo_queues(s, frame_samples, st, A, exact);
    if (rc != VK_OK) return rc;
    LaunchShape L;
    rc = plan_launch(s, p, acc, A, L);
    if (rc != VK_OK) return rc;
    if (use_order && !s->want_phase_stats) {
        rc = enqueue_tile_order(s, cam, p, g, L, st, A);
        if (rc != VK_OK) return rc;
    }
    if (adapt) {
        rc = enqueue_adaptive_compaction(acc, g, st, A);
        if (rc != VK_OK) return rc;
    }
    HIP_TRY(hipMemsetAsync(s->counter, 0, 32, st));       // work counter, this frame's clamped-sample count, per-launch unit counts
#ifdef VK_DEBUG_LIB
    if (s->want_phase_stats) rc = launch_phase_stats(s, L, st, A);
    else
#endif
    rc = launch_main(s, L, st, A);
    if (rc != VK_OK) return rc;
    // (an adaptive window with few active tiles is lopsided by construction: it must not strike the scene's dual launch off)
    if (adapt) s->dual.last = false;
    if (exact) {
        rc = enqueue_redo(s, A, L, n_pixels, st);
        if (rc != VK_OK) return rc;
    }
    rc = enqueue_resolve(A, p, g, d_out, acc, st);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->last_timed = true;
    return VK_OK;
}

// One device: render (f32) and, for RGB8 output, the fused output stage of this partition.
int enqueue_render_single(vk_scene *s, const vk_camera *cam, const vk_render_params *p, void *d_out, hipStream_t st, bool want_debug,
    vk_stats *stats, const AccumDesc *acc) {
    if (p->output_format == VK_OUTPUT_F32) return enqueue_render_f32(s, cam, p, reinterpret_cast<float *>(d_out), st, want_debug, stats, acc);
    HIP_TRY(hipSetDevice(s->device));
    int rc = s->fb.ensure((size_t)p->width * p->height * 3 * sizeof(float));
    if (rc != VK_OK) return rc;
    rc = enqueue_render_f32(s, cam, p, s->fb, st, want_debug, stats, acc);
    if (rc != VK_OK) return rc;
    return tile_move<TM_CONVERT_U8>(s->fb, d_out, p, TileGeom(p), st);
}

// Multi-device group: part j renders the tiles {t : t = R + W*(j + n*i)} of this call's partition (R of W) on its
// own device and stream, packs them into a slab (RGB8: through to_color, 4x smaller), the slab travels to devices[0] with
// ONE peer copy (xGMI), and devices[0] scatters the slabs into the caller's image on the caller's stream.  acc (progressive rendering):
// one descriptor per part, holding that part's running sums on its own device.
int enqueue_render_multi(vk_scene *grp, const vk_camera *cam, const vk_render_params *p, void *d_out, hipStream_t st0, vk_stats *stats,
    const AccumDesc *acc) {
    const uint32_t n = (uint32_t)grp->group.parts.size();
    const TileGeom g(p);
    const bool u8 = p->output_format == VK_OUTPUT_RGB8;
    const size_t slot_bytes = u8 ? 3 : 12;
    HIP_TRY(hipSetDevice(grp->device));
    HIP_TRY(hipEventRecord(grp->group.ev_begin, st0));      // the parts start after whatever the caller's stream held before this frame
    uint64_t samples = 0; uint32_t launches = 0;
    std::vector<TileGeom> geoms;
    std::vector<size_t> slab_size;
    for (uint32_t j = 0; j < n; j++) {
        vk_scene *q = grp->group.parts[j];
        vk_render_params pj = *p;
        pj.tile_rank = g.rank + g.world * j; pj.tile_world = g.world * n; pj.output_format = VK_OUTPUT_F32;
        const TileGeom gj(&pj);
        geoms.push_back(gj);
        HIP_TRY(hipSetDevice(q->device));
        HIP_TRY(hipStreamWaitEvent(q->group.stream, grp->group.ev_begin, 0));
        int rc = q->fb.ensure((size_t)p->width * p->height * 3 * sizeof(float));
        if (rc != VK_OK) return rc;
        vk_stats sj;
        memset(&sj, 0, sizeof(sj));
        rc = enqueue_render_f32(q, cam, &pj, q->fb, q->group.stream, false, &sj, acc ? &acc[j] : nullptr);
        if (rc != VK_OK) return rc;
        samples += sj.samples; launches += sj.kernel_launches;
        size_t bytes = (size_t)gj.n_local * 64u * slot_bytes;
        rc = q->group.slab.ensure(bytes);
        if (rc != VK_OK) return rc;
        rc = u8 ? tile_move<TM_PACK_U8>(q->fb, q->group.slab, &pj, gj, q->group.stream) : tile_move<TM_PACK_F32>(q->fb, q->group.slab, &pj, gj, q->group.stream);
        if (rc != VK_OK) return rc;
        if (bytes > q->group.landing.bytes()) {                // the landing buffer lives on devices[0]
            HIP_TRY(hipSetDevice(grp->device));
            rc = q->group.landing.ensure(bytes);
            if (rc != VK_OK) return rc;
            HIP_TRY(hipSetDevice(q->device));
        }
        slab_size.push_back(bytes);
        if (grp->group.comms.empty()) {
            if (bytes) HIP_TRY(hipMemcpyPeerAsync(q->group.landing, grp->device, q->group.slab, q->device, bytes, q->group.stream));
            HIP_TRY(hipEventRecord(q->group.ev_landed, q->group.stream));
        }
    }
    if (!grp->group.comms.empty()) {
        // The same exchange as ONE RCCL group: part j sends its slab on its own stream (behind its render and pack), devices[0] receives
        // the slabs on the group's receive stream, which waits for nothing but the start of the frame (the previous frame's unpack
        // kernels have read the landing buffers by then) — so the transfers overlap devices[0]'s own render.  ncclSend / ncclRecv pairs
        // inside one ncclGroupStart / ncclGroupEnd progress together; the receives complete in that stream's order, so ONE event says
        // that every slab has landed.  Part 0's slab is on devices[0] already and is unpacked where it lies.
        const RcclApi &R = rccl_api();
        vk_scene *q0 = grp->group.parts[0];
        HIP_TRY(hipSetDevice(q0->device));
        HIP_TRY(hipEventRecord(q0->group.ev_landed, q0->group.stream));
        HIP_TRY(hipStreamWaitEvent(grp->group.stream, grp->group.ev_begin, 0));
        RCCL_TRY(R.GroupStart());
        for (uint32_t j = 1; j < n; j++) {
            vk_scene *q = grp->group.parts[j];
            if (!slab_size[j]) continue;
            RCCL_TRY(R.Send(q->group.slab, slab_size[j], ncclUint8, 0, grp->group.comms[j], q->group.stream));
            RCCL_TRY(R.Recv(q->group.landing, slab_size[j], ncclUint8, (int)j, grp->group.comms[0], grp->group.stream));
        }
        RCCL_TRY(R.GroupEnd());
        HIP_TRY(hipSetDevice(grp->device));
        HIP_TRY(hipEventRecord(grp->group.ev_landed, grp->group.stream));
    }
    HIP_TRY(hipSetDevice(grp->device));
    for (uint32_t j = 0; j < n; j++) {
        vk_scene *q = grp->group.parts[j];
        vk_render_params pj = *p;
        pj.tile_rank = geoms[j].rank; pj.tile_world = geoms[j].world;
        const bool rccl = !grp->group.comms.empty();
        HIP_TRY(hipStreamWaitEvent(st0, (rccl && j != 0u ? grp : q)->group.ev_landed, 0));
        const void *from = rccl && j == 0u ? q->group.slab.get() : q->group.landing.get();
        int rc = u8 ? tile_move<TM_UNPACK_U8>(from, d_out, &pj, geoms[j], st0) : tile_move<TM_UNPACK_F32>(from, d_out, &pj, geoms[j], st0);
        if (rc != VK_OK) return rc;
    }
    grp->last_timed = true;
    if (stats) {
        stats->samples = samples; stats->kernel_launches = launches; stats->scene_in_lds = grp->group.parts[0]->plan.lds_bytes ? 1u : 0u;
        stats->kernel_ms = 0.0; stats->seconds = 0.0;
    }
    return VK_OK;
}

int enqueue_render(vk_scene *s, const vk_camera *cam, const vk_render_params *p, void *d_out, hipStream_t st, bool want_debug,
    vk_stats *stats, const AccumDesc *acc = nullptr) {
    int rc = check_render_args(s, cam, p);
    if (rc != VK_OK) return rc;
    if (!s->group.parts.empty()) {
        if (want_debug) return fail(VK_ERR_UNSUPPORTED, "per-sample debug output is single-device only");
        return enqueue_render_multi(s, cam, p, d_out, st, stats, acc);
    }
    return enqueue_render_single(s, cam, p, d_out, st, want_debug, stats, acc);
}

// (the communicators before the parts whose streams they use; every device resource goes with its owner: vk_resources.h)
void destroy_one(vk_scene *s) {
    if (!s) return;
    for (ncclComm_t c : s->group.comms) if (c) (void)rccl_api().CommDestroy(c);
    for (vk_scene *q : s->group.parts) destroy_one(q);
    delete s;
}

struct SceneDeleter { void operator()(vk_scene *s) const { destroy_one(s); } };
using ScenePtr = std::unique_ptr<vk_scene, SceneDeleter>;

int check_device(int device, hipDeviceProp_t &pr) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(VK_ERR_NO_DEVICE,
        "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(VK_ERR_BAD_ARG, "device index out of range");
    HIP_TRY(hipGetDeviceProperties(&pr, device));
    if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) return fail(VK_ERR_NO_DEVICE,
        std::string("device is ") + pr.gcnArchName + ", this build targets gfx950 only");
    return VK_OK;
}

// uploads an already linearised scene to one device
int create_on_device(const std::shared_ptr<const LinearScene> &host, int device, bool own_stream, ScenePtr &out) {
    hipDeviceProp_t pr;
    int rc = check_device(device, pr);
    if (rc != VK_OK) return rc;
    ScenePtr s(new vk_scene);
    s->device = device;
    s->host = host;
    s->env = EnvSwitches::read();
    HIP_TRY(hipSetDevice(device));
    s->num_cus = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    const LinearScene &H = *host;
    DScene &D = s->dev;
    memset(&D, 0, sizeof(D));
#define UP(vec, field) do { rc = upload(s.get(), H.vec, D.field); if (rc != VK_OK) return rc; } while (0)
    // LDS residency: items + spheres + accumulators must leave room for >= 2 workgroups per CU
    // (exact re-treeing: the second launch stages the tree as handed over instead of the rebuilt one, whichever is larger counts)
    size_t hot = std::max(H.items.size(), H.ref_items.size()) * sizeof(DItem) + H.spheres.size() * sizeof(DSphere) +
                 H.boxes.size() * sizeof(DBox);
    // Only the sphere-only kernels walk a rebuilt tree of exact re-treeing (segment_unsafe, the requeue, the grid build): a scene that runs
    // another instance (VK_FORCE_FULL_VARIANT=1) is uploaded with the tree as handed over (ref_items) in items[], for every launch of it
    const bool rebuilt = !H.ref_items.empty() && pick_variant(s.get()) == 0u;
    // the grid form (DGrid): the first launch stages the table [cells | refs] instead of a tree, the second one the tree as handed over
    bool grid = H.grid.nu != 0u && rebuilt && !s->env.no_grid;
    const size_t grid_table_bytes = grid ? ((H.grid_cells.size() + H.grid_refs.size()) * sizeof(uint32_t) + 31u) / 32u * 32u : 0u;
    // (the second launch and the diagnostic builds stage the tree as handed over, which therefore counts too where the scene is staged
    // in LDS; the probe of a grid view walks the grid like the frame's launch: launch_variant sends its COST launches to the GRID kernel)
    if (grid) hot = std::max(grid_table_bytes, std::max(H.ref_items.size(), H.items.size()) * sizeof(DItem)) + H.spheres.size() * sizeof(DSphere);
    s->plan.grid_on = grid;
    s->plan.hot_bytes = hot;
    plan_residency(s.get(), hot);
    if (grid && s->plan.lds_bytes == 0 && !s->env.grid_global) {
        // The grid form is for scenes staged in LDS.  From global memory every visited cell is three dependent cache misses (cell ->
        // references -> sphere) once the tables outgrow an XCD's L2, where a tree's top levels stay hot; and a large layer seen from far
        // away needs wide bands of cells around its primary rays (the dilation grows with the distance from the origin: 1.4 per 1 000).
        // Measured: 1 M spheres 500 against the near form's 1 280 Msamples/s, 160 000 spheres 850 against 1 290 (40 000: 1 930 against
        // 1 400, a win while everything fits L2: profiles/r05/experiments/README.md).
        grid = false;
        hot = std::max(H.items.size(), H.ref_items.size()) * sizeof(DItem) + H.spheres.size() * sizeof(DSphere) + H.boxes.size() * sizeof(DBox);
        s->plan.grid_on = false; s->plan.hot_bytes = hot;
        plan_residency(s.get(), hot);
    }
    D.gate_scale = 1.0f; D.tmin_gate = T_MIN;
    if (rebuilt) {
        // Exact re-treeing (vk_trace.h).  Staged in LDS: the rebuilt tree is the scene's, the tree as handed over serves the second launch
        // (`exact`).  Traversed from global memory: both trees in one array, early segments are walked again in place (DScene::walk_start).
        const DScene hv = H.host_view();
        D.t_pad = hv.t_pad; D.gate_scale = hv.gate_scale; D.tmin_gate = hv.tmin_gate;
        for (int k = 0; k < 3; k++) { D.trust_c0[k] = hv.trust_c0[k]; D.small_clo[k] = hv.small_clo[k]; D.small_chi[k] = hv.small_chi[k]; }
        D.trust_r0sq = hv.trust_r0sq;
        D.reach = hv.reach; D.clear_k = hv.clear_k; D.clear_r2 = hv.clear_r2; D.clear_slack = hv.clear_slack;
        if (grid) {
            // no ball, no reach: the grid's walk tests every sphere that can hold a candidate, wherever the ray starts
            use_grid(D);
            std::vector<uint32_t> table(grid_table_bytes / sizeof(uint32_t), 0u);
            std::copy(H.grid_cells.begin(), H.grid_cells.end(), table.begin());
            std::copy(H.grid_refs.begin(), H.grid_refs.end(), table.begin() + H.grid_cells.size());
            rc = upload(s.get(), table, D.grid_cells);
            if (rc != VK_OK) return rc;
            D.grid_refs = D.grid_cells + H.grid_cells.size();
            D.grid = H.grid;
            s->plan.grid_slots = (uint32_t)(grid_table_bytes / 32u);
        }
        if (!H.unit_item.empty() && H.proven) { rc = upload(s.get(), H.unit_item, D.unit_item); if (rc != VK_OK) return rc; }
        if (grid && s->plan.lds_bytes == 0) {
            // from global memory: the first launch reads the table and the spheres only; the tree as handed over serves the second one
            // (and the diagnostic builds)
            UP(ref_items, ref_items);
            D.items = D.ref_items; D.n_ref_items = hv.n_ref_items; D.n_items = D.n_ref_items; D.n_world_items = D.n_ref_items;
            D.unit_tree = D.ref_items;
            s->exact.on = true;
        } else
        if (s->plan.lds_bytes != 0) {
            UP(items, items); UP(ref_items, ref_items);
            D.n_ref_items = hv.n_ref_items; D.n_items = (uint32_t)H.items.size(); D.n_world_items = H.world_items;
            D.unit_tree = D.ref_items;
            s->exact.on = true;
        } else {
            uint32_t walk_start = 0;
            const std::vector<DItem> both = H.combined_items(walk_start);
            rc = upload(s.get(), both, D.items);
            if (rc != VK_OK) return rc;
            D.n_items = (uint32_t)both.size(); D.n_world_items = (uint32_t)both.size(); D.walk_start = walk_start;
            D.unit_tree = D.items;       // (the tree as handed over comes first, item for item)
        }
    } else if (!H.ref_items.empty()) {
        UP(ref_items, items);        // (the tree as handed over, as s->exact.ref_view has it)
        D.n_items = (uint32_t)H.ref_items.size(); D.n_world_items = D.n_items;
    } else {
        UP(items, items);
        D.n_items = (uint32_t)H.items.size(); D.n_world_items = H.world_items;
    }
    UP(spheres, spheres); UP(sphere_mat, sphere_mat); UP(moving, moving); UP(rects, rects); UP(boxes, boxes);
    UP(lists, lists); UP(list_refs, list_refs); UP(media, media); UP(instances, instances);
    UP(materials, materials); UP(sphere_material, sphere_material); UP(textures, textures); UP(images, images);
    UP(image_bytes, image_bytes);
    UP(perlins, perlins); UP(lights, lights);
    if (!H.tie_rank.empty() && (rebuilt || H.ref_items.empty())) UP(tie_rank, tie_rank);
#undef UP
    D.tie_base_rect = H.tie_base_rect; D.tie_base_box = H.tie_base_box; D.tie_base_list = H.tie_base_list;
    D.fast_div = H.host_view().fast_div;
    D.n_noise_spheres = H.n_noise_spheres;
    for (int k = 0; k < 4; k++) { D.noise_sphere[k] = H.noise_sphere[k]; D.noise_tex[k] = H.noise_tex[k];
        D.noise_perlin[k] = H.noise_perlin[k]; }
    D.n_spheres = (uint32_t)H.spheres.size();
    D.n_lights = (uint32_t)H.lights.size(); D.features = H.features; D.n_boxes = (uint32_t)H.boxes.size();
#define MAKE(expr) do { rc = (expr); if (rc != VK_OK) return rc; } while (0)
    MAKE(s->counter.ensure(256));
    MAKE(s->ev0.create());
    MAKE(s->ev1.create());
    if (own_stream) {
        MAKE(s->group.stream.create());
        MAKE(s->group.ev_landed.create(hipEventDisableTiming));
    }
    if (s->exact.on) {
        s->exact.ref_view = handed_over_view(D);      // the second launch's scene
        MAKE(s->exact.redo_count.ensure((REDO_REGIONS * REDO_COUNT_STRIDE + 16) * sizeof(uint32_t)));
        HIP_TRY(s->exact.plan_host.alloc(8 * sizeof(uint32_t)));
        MAKE(s->exact.ev_plan[0].create(hipEventDisableTiming));
        MAKE(s->exact.ev_plan[1].create(hipEventDisableTiming));
    }
    if (s->plan.dual_launch) {
        MAKE(s->dual.stream2.create());
        MAKE(s->dual.ev_fork.create(hipEventDisableTiming));
        MAKE(s->dual.ev_join.create(hipEventDisableTiming));
    }
#undef MAKE
    out = std::move(s);
    return VK_OK;
}

int linearize_desc(const vk_scene_desc *desc, std::shared_ptr<const LinearScene> &out) {
    auto h = std::make_shared<LinearScene>();
    std::string err;
    LinearizeOptions opt;
    opt.retree = EnvSwitches::read().retree;
    // VK_GATE_PROOF=0: among the trees the description allows, prefer the empirical form (comparisons, the constructed counter-example on
    // the device).  It does NOT allow an unproven tree by itself: that takes VK_SCENE_EMPIRICAL_TREES in the description.
    if (const char *e = getenv("VK_GATE_PROOF")) opt.want_proof = e[0] != '0';
#ifdef VK_DEBUG_LIB
    // unsound test switches (LinearizeOptions): the debug build only; the product's trees are the proven one, the handed-over one, or
    // what the description's flags opt into
    if (const char *e = getenv("VK_GATE_GROW")) opt.gate_grow = e[0] != '0';
    if (const char *e = getenv("VK_T_PAD")) opt.t_pad = (float)atof(e);
    if (const char *e = getenv("VK_EMPIRICAL_TREES")) opt.allow_empirical = e[0] == '1';
    if (const char *e = getenv("VK_NEAR_FORM")) opt.near_form = e[0] != '0';
    if (const char *e = getenv("VK_UNIT_FORM")) opt.unit_form = e[0] != '0';
    if (const char *e = getenv("VK_NEAR_FIRST")) opt.near_first = e[0] != '0';
#endif
    int rc = linearize(desc, *h, err, opt);
    if (rc != VK_OK) return fail(rc, err);
    out = h;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_abi_version(void) { return VK_ABI_VERSION; }

int vk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, i) == hipSuccess && strncmp(pr.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

const char *vk_last_error(void) { return g_err.c_str(); }

int vk_gather_backends(void) { return 1 | (rccl_api().ok() ? 2 : 0); }

int vk_scene_create(const vk_scene_desc *desc, int device, vk_scene **out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null out pointer");
    *out = nullptr;
    return guarded([&]() -> int {
        hipDeviceProp_t pr;
        int rc = check_device(device, pr);           // before the (possibly long) linearisation
        if (rc != VK_OK) return rc;
        std::shared_ptr<const LinearScene> host;
        rc = linearize_desc(desc, host);
        if (rc != VK_OK) return rc;
        ScenePtr s;
        rc = create_on_device(host, device, false, s);
        if (rc != VK_OK) return rc;
        *out = s.release();
        return VK_OK;
    });
}

int vk_scene_create_multi(const vk_scene_desc *desc, const int *devices, int n_devices, vk_scene **out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null out pointer");
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return fail(VK_ERR_BAD_ARG, "devices: need 1..64 entries");
    return guarded([&]() -> int {
        hipDeviceProp_t pr;
        for (int j = 0; j < n_devices; j++) { int rc = check_device(devices[j], pr); if (rc != VK_OK) return rc; }
        std::shared_ptr<const LinearScene> host;
        int rc = linearize_desc(desc, host);
        if (rc != VK_OK) return rc;
        ScenePtr grp(new vk_scene);
        grp->device = devices[0];
        grp->host = host;
        grp->env = EnvSwitches::read();
        memset(&grp->dev, 0, sizeof(grp->dev));
        for (int j = 0; j < n_devices; j++) {
            ScenePtr part;
            rc = create_on_device(host, devices[j], true, part);
            if (rc != VK_OK) return rc;
            if (devices[j] != devices[0]) {          // let devices[0] and this device address each other's memory (xGMI peer copies)
                int can = 0;
                HIP_TRY(hipDeviceCanAccessPeer(&can, devices[j], devices[0]));
                if (!can)
                    fprintf(stderr, "vecchio_amd: device %d cannot address device %d's memory (no peer access): its tile slab travels "
                        "through host memory\n", devices[j], devices[0]);
                if (can) {
                    HIP_TRY(hipSetDevice(devices[j]));
                    hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(VK_ERR_HIP,
                        std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
                    (void)hipGetLastError();
                }
            }
            grp->group.parts.push_back(part.release());
        }
        const bool want_rccl = (desc->flags & VK_SCENE_RCCL_GATHER) != 0u || (getenv("VK_MULTI_GATHER") && !strcmp(getenv("VK_MULTI_GATHER"), "rccl"));
        if (want_rccl) {
            // one communicator rank per DEVICE: a device listed twice (the one-GPU test shape) cannot take part
            bool distinct = true;
            for (int a = 0; a < n_devices; a++) for (int b = a + 1; b < n_devices; b++) distinct = distinct && devices[a] != devices[b];
#ifdef VK_DEBUG_LIB
            if (getenv("VK_RCCL_ALLOW_DUPLICATE_DEVICES")) distinct = true;      // (with the test double of VK_RCCL_LIB only: real RCCL refuses)
#endif
            const RcclApi &R = rccl_api();
            if (!R.ok()) fprintf(stderr, "vecchio_amd: VK_SCENE_RCCL_GATHER: %s; the tile slabs travel by peer copies\n", R.why.c_str());
            else if (!distinct) fprintf(stderr, "vecchio_amd: VK_SCENE_RCCL_GATHER: a device is listed more than once (one communicator rank per "
                "device); the tile slabs travel by peer copies\n");
            else {
                grp->group.comms.assign((size_t)n_devices, nullptr);
                ncclResult_t r = R.CommInitAll(grp->group.comms.data(), n_devices, devices);
                if (r != ncclSuccess) {
                    fprintf(stderr, "vecchio_amd: ncclCommInitAll over %d devices failed (%s); the tile slabs travel by peer copies\n", n_devices,
                        R.GetErrorString(r));
                    grp->group.comms.clear();
                }
            }
            if (!grp->group.comms.empty()) {       // the receive stream of devices[0] and the event behind the frame's last receive
                HIP_TRY(hipSetDevice(devices[0]));
                if ((rc = grp->group.stream.create()) != VK_OK) return rc;
                if ((rc = grp->group.ev_landed.create(hipEventDisableTiming)) != VK_OK) return rc;
            }
        }
        HIP_TRY(hipSetDevice(devices[0]));
        if ((rc = grp->group.ev_begin.create(hipEventDisableTiming)) != VK_OK) return rc;
        grp->plan.lds_bytes = grp->group.parts[0]->plan.lds_bytes; grp->plan.hot_bytes = grp->group.parts[0]->plan.hot_bytes;
        *out = grp.release();
        return VK_OK;
    });
}

void vk_scene_destroy(vk_scene *s) { destroy_one(s); }

int vk_scene_get_info(const vk_scene *s, vk_scene_info *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    const LinearScene &H = *s->host;
    const vk_scene *one = first_part(s);
    out->n_items = (uint32_t)H.items.size();
    out->n_prims = H.n_prims;
    out->n_instances = (uint32_t)H.instances.size();
    uint64_t b = 0;
    b += H.items.size() * sizeof(DItem) + H.spheres.size() * (sizeof(DSphere) + 4) + H.moving.size() * sizeof(DMoving) +
         H.rects.size() * sizeof(DRect) + H.lists.size() * sizeof(DList) + H.list_refs.size() * 4 +
         H.media.size() * sizeof(DMedium) + H.instances.size() * sizeof(DInstance) + H.materials.size() * sizeof(DMaterial) +
         H.textures.size() * sizeof(DTexture) + H.image_bytes.size() + H.perlins.size() * sizeof(DPerlin);
    out->device_bytes = b;
    out->lds_bytes = one->plan.lds_bytes;
    out->features = pick_variant(one);
    const bool rebuilt = !H.ref_items.empty() && pick_variant(one) == 0u;      // (see create_on_device)
    out->tree = rebuilt ? (one->plan.grid_on ? VK_TREE_REBUILT_GRID : H.near_form ? VK_TREE_REBUILT_NEAR : (H.proven ? VK_TREE_REBUILT_PROVEN : VK_TREE_REBUILT_EMPIRICAL))
                                     : (!H.tie_rank.empty() && H.ref_items.empty() ? VK_TREE_REBUILT_FAST : VK_TREE_HANDED_OVER);
    out->gather = s->group.parts.empty() ? VK_GATHER_NONE : (s->group.comms.empty() ? VK_GATHER_PEER_COPY : VK_GATHER_RCCL);
    out->tree_suspended_frames = 0;
    for (const vk_scene *q : (s->group.parts.empty() ? std::vector<vk_scene *>{const_cast<vk_scene *>(s)} : s->group.parts))
        if (q->exact.resume > q->exact.frame_no + 1u) out->tree_suspended_frames = std::max<uint32_t>(out->tree_suspended_frames,
            (uint32_t)(q->exact.resume - q->exact.frame_no - 1u));
    return VK_OK;
}

int vk_render_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, void *d_rgb_out, void *hip_stream,
    vk_stats *stats_out) {
    if (!d_rgb_out) return fail(VK_ERR_BAD_ARG, "null device framebuffer");
    return guarded([&]() -> int { return enqueue_render(scene, cam, params, d_rgb_out, reinterpret_cast<hipStream_t>(hip_stream), false,
        stats_out); });
}

// HIP-event time (ms) of the launches enqueued by the last vk_render_device / vk_render on
// this scene; synchronises on their end event.  Multi-device: the slowest part.
int vk_scene_part_info(vk_scene *s, int part, vk_part_info *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    const int n = s->group.parts.empty() ? 1 : (int)s->group.parts.size();
    if (part < 0 || part >= n) return fail(VK_ERR_BAD_ARG, "part index out of range");
    vk_scene *q = s->group.parts.empty() ? s : s->group.parts[(size_t)part];
    memset(out, 0, sizeof(*out));
    out->n_parts = (uint32_t)n;
    out->device = q->device;
    hipDeviceProp_t pr;
    HIP_TRY(hipGetDeviceProperties(&pr, q->device));
    snprintf(out->name, sizeof(out->name), "%s", pr.name);
    if (hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof(out->pci_bus_id), q->device) != hipSuccess) { (void)hipGetLastError(); out->pci_bus_id[0] = 0; }
    const int landing = s->group.parts.empty() ? q->device : s->device;
    int can = 1;
    if (q->device != landing) HIP_TRY(hipDeviceCanAccessPeer(&can, q->device, landing));
    out->can_access_landing_device = (uint32_t)can;
    out->kernel_ms = -1.0;
    if (q->last_timed) {
        double ms = 0.0;
        int rc = vk_scene_last_kernel_ms(q, &ms);
        if (rc != VK_OK) return rc;
        out->kernel_ms = ms;
    }
    return VK_OK;
}

int vk_scene_last_kernel_ms(vk_scene *s, double *ms_out) {
    if (!s || !ms_out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!s->last_timed) return fail(VK_ERR_BAD_ARG, "no render enqueued yet");
    if (!s->group.parts.empty()) {
        double worst = 0.0;
        for (vk_scene *q : s->group.parts) {
            double ms = 0.0;
            int rc = vk_scene_last_kernel_ms(q, &ms);
            if (rc != VK_OK) return rc;
            if (ms > worst) worst = ms;
        }
        *ms_out = worst;
        return VK_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->ev1));
    if (s->wave_times && s->group.parts.empty()) {      // diagnostics: when the waves of the last render's FIRST launch started, pulled their last unit and ended
        std::vector<unsigned long long> w(3u * 1024u * 16u);
        HIP_TRY(hipMemcpy(w.data(), s->wave_times, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0; std::vector<double> ends, lasts;
        for (size_t k = 0; k < w.size(); k += 3) if (w[k]) { t0 = std::min(t0, w[k]); t1 = std::max(t1, w[k + 2]); }
        for (size_t k = 0; k < w.size(); k += 3) if (w[k]) { ends.push_back((double)(w[k + 2] - t0) * 1e-5); lasts.push_back((double)(w[k + 1] - t0) * 1e-5); }
        std::sort(ends.begin(), ends.end()); std::sort(lasts.begin(), lasts.end());
        if (!ends.empty()) {
            auto q = [&](const std::vector<double> &v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
            fprintf(stderr, "vecchio_amd: %zu waves, span %.2f ms; wave ends (ms): 1%% %.2f 10%% %.2f 50%% %.2f 90%% %.2f 99%% %.2f max %.2f; last unit pull: 50%% %.2f 99%% %.2f max %.2f\n",
                ends.size(), (double)(t1 - t0) * 1e-5, q(ends, 0.01), q(ends, 0.1), q(ends, 0.5), q(ends, 0.9), q(ends, 0.99), ends.back(), q(lasts, 0.5), q(lasts, 0.99), lasts.back());
        }
    }
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    *ms_out = (double)ms;
    if (s->dual.last && s->plan.dual_launch) {        // did the two launches of the last frame share the work?  (see vk_scene::Dual::strikes)
        uint32_t u[2] = {0u, 0u};
        if (hipMemcpy(u, s->counter + 4, sizeof(u), hipMemcpyDeviceToHost) == hipSuccess && u[0] + u[1] > 0u) {
            const double share = (double)u[1] / (double)(u[0] + u[1]);       // ~12 / 28 when both run side by side
            const bool lopsided = share < 0.10 || share > 0.90;
            s->dual.strikes = lopsided ? s->dual.strikes + 1 : 0;
            if (s->env.dual_debug)
                fprintf(stderr, "vecchio_amd: dual launch: 1024-thread launch %u units, 768-thread launch %u units (%.2f)\n", u[0], u[1],
                    share);
            if (s->dual.strikes >= 2) {
                s->plan.dual_launch = false;
                fprintf(stderr, "vecchio_amd: the two launches of the 7-waves-per-SIMD shape do not run side by side on this runtime "
                                "(unit split %u / %u); using the single-launch shape from now on\n", u[0], u[1]);
            }
        }
        (void)hipGetLastError();
        s->dual.last = false;
    }
    return VK_OK;
}

// Samples of the last render whose radiance was clamped on its way into the fixed-point pixel sums; waits for the render's end.
int vk_scene_last_clamped_samples(vk_scene *s, uint64_t *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!s->last_timed) return fail(VK_ERR_BAD_ARG, "no render enqueued yet");
    *out = 0;
    if (!s->group.parts.empty()) {
        for (vk_scene *q : s->group.parts) {
            uint64_t v = 0;
            int rc = vk_scene_last_clamped_samples(q, &v);
            if (rc != VK_OK) return rc;
            *out += v;
        }
        return VK_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->ev1));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, reinterpret_cast<unsigned long long *>(s->counter.get()) + 1, sizeof(v), hipMemcpyDeviceToHost));
    *out = v;
    return VK_OK;
}

// Exact re-treeing: samples of the last render that the first launch handed to the second one (rendered on the tree as handed
// over); waits for the render's end.  A frame whose queues overflowed is complete all the same (the fallback launch rendered it on the
// tree as handed over: enqueue_render_f32); it counts as entirely requeued.
int vk_scene_last_requeued_samples(vk_scene *s, uint64_t *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!s->last_timed) return fail(VK_ERR_BAD_ARG, "no render enqueued yet");
    *out = 0;
    if (!s->group.parts.empty()) {
        int worst = VK_OK;
        for (vk_scene *q : s->group.parts) {
            uint64_t v = 0;
            int rc = vk_scene_last_requeued_samples(q, &v);
            if (rc != VK_OK) worst = rc;
            *out += v;
        }
        return worst;
    }
    if (!s->exact.redo_last) return VK_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->ev1));
    if (!s->exact.plan_copied) {      // (the caller ran more than two frames ahead: this frame's plan was not copied; read it now)
        uint32_t plan[4];
        HIP_TRY(hipMemcpy(plan, s->exact.redo_count + REDO_REGIONS * REDO_COUNT_STRIDE, sizeof(plan), hipMemcpyDeviceToHost));
        *out = plan[2] != 0u ? s->exact.redo_last_samples : plan[1];
        return VK_OK;
    }
    const int b = s->exact.plan_last;
    *out = s->exact.plan_host[4 * b + 2] != 0u ? s->exact.redo_last_samples : s->exact.plan_host[4 * b + 1];
    judge_arrived_frames(s);
    return VK_OK;
}

static int render_host(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, void *out_host, vk_stats *stats_out,
    float *debug_out, const AccumDesc *acc = nullptr) {
    if (!out_host) return fail(VK_ERR_BAD_ARG, "null framebuffer");
    int rc = check_render_args(scene, cam, params);
    if (rc != VK_OK) return rc;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(scene->device));
    const bool u8 = params->output_format == VK_OUTPUT_RGB8;
    size_t n_pixels = (size_t)params->width * params->height;
    size_t bytes = n_pixels * 3 * (u8 ? 1 : sizeof(float));
    // a multi-device group scatters into the image on devices[0]; a single device renders f32 into fb and converts into fb8
    void *d_img;
    if (u8) { rc = scene->fb8.ensure(bytes); d_img = scene->fb8; }
    else { rc = scene->fb.ensure(bytes); d_img = scene->fb; }
    if (rc != VK_OK) return rc;
    vk_stats st;
    double ms = 0.0;
    {
        memset(&st, 0, sizeof(st));
        rc = enqueue_render(scene, cam, params, d_img, nullptr, debug_out != nullptr, &st, acc);
        if (rc != VK_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        uint64_t requeued = 0;
        rc = vk_scene_last_requeued_samples(scene, &requeued);      // (judges the frame: see vk_scene::Exact::resume)
        if (rc != VK_OK) return rc;
    }
    rc = vk_scene_last_kernel_ms(scene, &ms);
    if (rc != VK_OK) return rc;
    st.kernel_ms = ms;
    rc = vk_scene_last_clamped_samples(scene, &st.clamped_samples);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    uint32_t world = params->tile_world ? params->tile_world : 1;
    if (world == 1) {
        HIP_TRY(hipMemcpy(out_host, d_img, bytes, hipMemcpyDeviceToHost));     // the ONE device-to-host copy of the frame
    } else {
        // a partial image: only this call's tiles may be touched in the caller's buffer
        std::vector<uint8_t> tmp(bytes);
        HIP_TRY(hipMemcpy(tmp.data(), d_img, bytes, hipMemcpyDeviceToHost));
        uint32_t tiles_x = (params->width + TILE - 1) / TILE;
        const size_t px_bytes = u8 ? 3 : 12;
        uint8_t *dst = reinterpret_cast<uint8_t *>(out_host);
        for (uint32_t y = 0; y < params->height; y++)
            for (uint32_t x = 0; x < params->width; x++) {
                uint32_t tile = (y / TILE) * tiles_x + (x / TILE);
                if (tile % world != params->tile_rank) continue;
                uint32_t row = u8 ? params->height - 1 - y : y;                  // RGB8 images are top-down
                size_t i = ((size_t)row * params->width + x) * px_bytes;
                memcpy(dst + i, tmp.data() + i, px_bytes);
            }
    }
    if (debug_out) HIP_TRY(hipMemcpy(debug_out, scene->debug, n_pixels * params->samples_per_pixel * sizeof(float4),
        hipMemcpyDeviceToHost));
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats_out) *stats_out = st;
    return VK_OK;
}

int vk_render(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, float *rgb_out, vk_stats *stats_out) {
    return guarded([&]() -> int { return render_host(scene, cam, params, rgb_out, stats_out, nullptr); });
}

// test hook: as vk_render, also returning every sample: samples_out[(pixel*spp + s)*4 + 0..2]
// = radiance before the finite filter, [+3] = the sample's draw count (bit pattern)
int vk_debug_render_samples(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, float *rgb_out, float *samples_out) {
    if (!samples_out) return fail(VK_ERR_BAD_ARG, "null samples buffer");
    if (params && params->output_format != VK_OUTPUT_F32) return fail(VK_ERR_BAD_ARG, "per-sample debug output needs VK_OUTPUT_F32");
    return guarded([&]() -> int { return render_host(scene, cam, params, rgb_out, nullptr, samples_out); });
}

// test hook: the render_kernel launches of the scene's last frame (vk_scene::launch_log)
int vk_debug_last_launches(vk_scene *scene, vk_debug_launch *out, uint32_t cap, uint32_t *n) {
    if (!scene || !n || (cap && !out)) return fail(VK_ERR_BAD_ARG, "null argument");
    std::vector<vk_debug_launch> all;
    for (const vk_scene *q : (scene->group.parts.empty() ? std::vector<vk_scene *>{scene} : scene->group.parts))
        all.insert(all.end(), q->launch_log.begin(), q->launch_log.end());
    *n = (uint32_t)all.size();
    for (uint32_t k = 0; k < cap && k < *n; k++) out[k] = all[k];
    return VK_OK;
}

}  // extern "C"

// ---- first-hit buffers (vk_render_aov): one launch of aov_kernel on the scene's device (devices[0] of a multi-device scene), on its own
// events and output buffers.  Nothing that describes vk_render's last frame (events, counters, launch log, verdicts on the rebuilt tree) is
// read or written, and no progress handle's sums.
namespace {

// The tree the first-hit walk runs on: the tree as handed over.  Where the scene has a second launch (exact re-treeing staged in LDS, or
// the grid form) that is s->exact.ref_view, the REDO launch's view; where both trees share items[] (exact re-treeing from global memory) it is
// their first part, whose exits lead past the rebuilt tree (vk_linearize.cpp combined_items) — the in-place redo walk's tree.  Anywhere
// else the scene holds one tree: the one handed over, or under VK_SCENE_FAST_ACCEL the rebuilt one (with its tie table), which is then
// also what vk_render walks — such a scene has no copy of the tree as handed over on the device.
DScene aov_view(const vk_scene *s) { return s->exact.on ? s->exact.ref_view : handed_over_view(s->dev); }

// aov_view for a launcher: none of these kernels knows the rebuilt forms' gates.  what: the walk that asks, as the refusal names it.
int query_view(const vk_scene *q, const char *what, DScene *S) {
    *S = aov_view(q);
    if (!is_plain_tree_view(*S))
        return fail(VK_ERR_BAD_ARG, std::string("internal error: ") + what + " needs a tree view without the rebuilt forms' gates");
    return VK_OK;
}

// n_bufs: 4 (vk_render_aov) or 5 (vk_render_guides: bounces too)
int check_aov_args(vk_scene *scene, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, const void *const *bufs,
    int n_bufs) {
    int rc = check_call_args(scene, cam, p);
    if (rc != VK_OK) return rc;
    if (p->output_format != VK_OUTPUT_F32) return fail(VK_ERR_BAD_ARG, "first-hit buffers are f32 only (output_format must be VK_OUTPUT_F32)");
    // (vk_render_guides has refused five null buffers already, before it looked at the scene: check_guide_args)
    if (n_bufs == 4 && !bufs[0] && !bufs[1] && !bufs[2] && !bufs[3]) return fail(VK_ERR_BAD_ARG, "no first-hit buffer wanted (all four are null)");
    if ((uint64_t)first_sample + p->samples_per_pixel > 0xFFFFFFFFull) return fail(VK_ERR_BAD_ARG,
        "first_sample + samples_per_pixel exceeds 2^32 - 1");
    return VK_OK;
}

// floats per pixel of albedo, normal, depth, coverage (and vk_render_guides' bounces)
constexpr uint32_t AOV_COMPONENTS[5] = {3u, 3u, 1u, 1u, 1u};

// gp != nullptr: the specular guides (specular_guides_kernel) with d_bounces as the fifth buffer, otherwise the first-hit buffers
int enqueue_aov(vk_scene *q, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, float *const d[4], hipStream_t st,
    bool timed, const vk_guide_params *gp = nullptr, float *d_bounces = nullptr) {
    HIP_TRY(hipSetDevice(q->device));
    const TileGeom g(p);
    AovArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "the first-hit walk", &A.S);
    if (rc != VK_OK) return rc;
    A.C.cam = *cam;
    A.C.width = p->width; A.C.height = p->height; A.C.spp = p->samples_per_pixel; A.C.max_depth = 0u;
    A.C.seed = p->seed; A.C.integrator = p->integrator; A.C.background = p->background;
    A.C.bg[0] = p->background_color[0]; A.C.bg[1] = p->background_color[1]; A.C.bg[2] = p->background_color[2];
    A.albedo = d[0]; A.normal = d[1]; A.depth = d[2]; A.coverage = d[3];
    A.first_sample = first_sample; A.tiles_x = g.tiles_x; A.tile_rank = g.rank; A.tile_world = g.world; A.n_local = g.n_local;
    if (timed) {
        rc = q->aov.ev0.create();
        if (rc == VK_OK) rc = q->aov.ev1.create();
        if (rc != VK_OK) return rc;
        HIP_TRY(hipEventRecord(q->aov.ev0, st));
    }
    if (g.n_local != 0u) {
        const dim3 grid((g.n_local + AOV_BLOCK / 64 - 1) / (AOV_BLOCK / 64));
        if (gp) {
            GuideArgs G;
            G.A = A; G.bounces = d_bounces; G.max_bounces = gp->max_bounces; G.fuzz_max = gp->fuzz_max;
            with_walk_variant(q->host->features, [&](auto f) {
                hipLaunchKernelGGL(specular_guides_kernel<decltype(f)::value>, grid, dim3(AOV_BLOCK), 0, st, G);
            });
        } else {
            with_walk_variant(q->host->features, [&](auto f) {
                hipLaunchKernelGGL(aov_kernel<decltype(f)::value>, grid, dim3(AOV_BLOCK), 0, st, A);
            });
        }
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(q->aov.ev1, st));
    return VK_OK;
}

void aov_stats(const vk_render_params *p, vk_stats *st) {
    const TileGeom g(p);
    memset(st, 0, sizeof(*st));
    st->samples = partition_samples(p, g);
    st->kernel_launches = g.n_local != 0u ? 1u : 0u;
}

// ---- the host-pointer calls (vk_render_aov, vk_render_guides, vk_denoise, vk_temporal_accumulate): the call's images side by side in ONE
// staging buffer of the handle, uploads, a timed launch between two events, downloads, vk_stats.
struct StagedImages {
    float *dev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // image k's slice; null for a null image
    // Lays the non-null images host[0, n) (comps[k] floats per pixel) out in `buf`, grown as needed, and uploads those whose bit is set
    // in `mask`.  The buffer's device must be current.
    int upload(DeviceBuffer<float> &buf, float *const *host, const uint32_t *comps, int n, size_t n_pixels, uint32_t mask) {
        host_ = host; comps_ = comps; n_ = n; n_pixels_ = n_pixels;
        size_t floats = 0;
        for (int k = 0; k < n; k++) if (host[k]) floats += n_pixels * comps[k];
        int rc = buf.ensure(floats * sizeof(float));
        if (rc != VK_OK) return rc;
        size_t at = 0;
        for (int k = 0; k < n; k++) {
            if (!host[k]) continue;
            dev[k] = buf + at; at += n_pixels * comps[k];
            if (mask >> k & 1u) HIP_TRY(hipMemcpy(dev[k], host[k], n_pixels * comps[k] * sizeof(float), hipMemcpyHostToDevice));
        }
        return VK_OK;
    }
    // the images whose bit is set in `mask`, back into the caller's memory (waits for the launch: the copies are synchronous)
    int download(uint32_t mask) const {
        for (int k = 0; k < n_; k++)
            if (host_[k] && (mask >> k & 1u)) HIP_TRY(hipMemcpy(host_[k], dev[k], n_pixels_ * comps_[k] * sizeof(float), hipMemcpyDeviceToHost));
        return VK_OK;
    }

private:
    float *const *host_ = nullptr; const uint32_t *comps_ = nullptr; int n_ = 0; size_t n_pixels_ = 0;
};

// ends a timed host-pointer call: waits for its closing event and writes the two times into the caller's stats (whose counts are filled)
int end_timed_call(hipEvent_t ev0, hipEvent_t ev1, std::chrono::steady_clock::time_point t0, vk_stats *stats_out) {
    HIP_TRY(hipEventSynchronize(ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats_out) {
        stats_out->kernel_ms = (double)ms;
        stats_out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return VK_OK;
}

// The host-pointer call of vk_render_aov (n_bufs 4, gp null) and vk_render_guides (n_bufs 5): the wanted buffers staged side by side in the
// scene's own device buffer, one timed launch, the copies back.  The arguments have been checked.
int render_aov_host(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample, float *const host[5],
    int n_bufs, const vk_guide_params *gp, vk_stats *stats_out) {
    const auto t0 = std::chrono::steady_clock::now();
    vk_scene *q = first_part(scene);
    HIP_TRY(hipSetDevice(q->device));
    // a partition: the caller's pixels outside it must come back untouched
    const bool partial = (params->tile_world ? params->tile_world : 1u) > 1u;
    StagedImages im;
    int rc = im.upload(q->aov.buf, host, AOV_COMPONENTS, n_bufs, (size_t)params->width * params->height, partial ? ~0u : 0u);
    if (rc != VK_OK) return rc;
    rc = enqueue_aov(q, cam, params, first_sample, im.dev, nullptr, true, gp, im.dev[4]);
    if (rc != VK_OK) return rc;
    if ((rc = im.download(~0u)) != VK_OK) return rc;
    if (stats_out) aov_stats(params, stats_out);
    return end_timed_call(q->aov.ev0, q->aov.ev1, t0, stats_out);
}

// vk_render_guides' own checks, made first (they need no scene), then the first-hit checks with five buffers
int check_guide_args(vk_scene *scene, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, const vk_guide_params *gp,
    const void *const bufs[5]) {
    if (!gp) return fail(VK_ERR_BAD_ARG, "null guide parameters");
    if (gp->max_bounces > 8u) return fail(VK_ERR_BAD_ARG, "guide max_bounces exceeds 8");
    if (!(gp->fuzz_max >= 0.0f) || !(gp->fuzz_max < INFINITY)) return fail(VK_ERR_BAD_ARG, "guide fuzz_max must be finite and >= 0");
    if (gp->flags != 0u) return fail(VK_ERR_BAD_ARG, "guide flags must be 0");
    if (!bufs[0] && !bufs[1] && !bufs[2] && !bufs[3] && !bufs[4]) return fail(VK_ERR_BAD_ARG, "no guide buffer wanted (all five are null)");
    return check_aov_args(scene, cam, p, first_sample, bufs, 5);
}

}  // namespace

extern "C" {

int vk_render_aov(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample, float *albedo, float *normal,
    float *depth, float *coverage, vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *host[5] = {albedo, normal, depth, coverage, nullptr};
        int rc = check_aov_args(scene, cam, params, first_sample, reinterpret_cast<const void *const *>(host), 4);
        if (rc != VK_OK) return rc;
        return render_aov_host(scene, cam, params, first_sample, host, 4, nullptr, stats_out);
    });
}

int vk_render_aov_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample, void *d_albedo,
    void *d_normal, void *d_depth, void *d_coverage, void *hip_stream, vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *dev[4] = {static_cast<float *>(d_albedo), static_cast<float *>(d_normal), static_cast<float *>(d_depth),
                         static_cast<float *>(d_coverage)};
        int rc = check_aov_args(scene, cam, params, first_sample, reinterpret_cast<const void *const *>(dev), 4);
        if (rc != VK_OK) return rc;
        vk_scene *q = first_part(scene);
        rc = enqueue_aov(q, cam, params, first_sample, dev, reinterpret_cast<hipStream_t>(hip_stream), false);
        if (rc != VK_OK) return rc;
        if (stats_out) aov_stats(params, stats_out);
        return VK_OK;
    });
}

}  // extern "C"

// ---- specular guides (vk_render_guides): vk_render_aov's launcher, checks, events and staging buffer around specular_guides_kernel
extern "C" {

int vk_guide_default_params(vk_guide_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null guide parameters");
    out->max_bounces = 4u; out->fuzz_max = 0.0f; out->flags = 0u;
    return VK_OK;
}

int vk_render_guides(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
    const vk_guide_params *gp, float *albedo, float *normal, float *depth, float *coverage, float *bounces, vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *host[5] = {albedo, normal, depth, coverage, bounces};
        int rc = check_guide_args(scene, cam, params, first_sample, gp, reinterpret_cast<const void *const *>(host));
        if (rc != VK_OK) return rc;
        return render_aov_host(scene, cam, params, first_sample, host, 5, gp, stats_out);
    });
}

int vk_render_guides_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
    const vk_guide_params *gp, void *d_albedo, void *d_normal, void *d_depth, void *d_coverage, void *d_bounces, void *hip_stream,
    vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *dev[5] = {static_cast<float *>(d_albedo), static_cast<float *>(d_normal), static_cast<float *>(d_depth),
                         static_cast<float *>(d_coverage), static_cast<float *>(d_bounces)};
        int rc = check_guide_args(scene, cam, params, first_sample, gp, reinterpret_cast<const void *const *>(dev));
        if (rc != VK_OK) return rc;
        vk_scene *q = first_part(scene);
        rc = enqueue_aov(q, cam, params, first_sample, dev, reinterpret_cast<hipStream_t>(hip_stream), false, gp, dev[4]);
        if (rc != VK_OK) return rc;
        if (stats_out) aov_stats(params, stats_out);
        return VK_OK;
    });
}

}  // extern "C"

// ---- ray-batch queries (vk_trace_rays, vk_trace_occluded, vk_trace_radiance, vk_trace_irradiance, vk_trace_probes, vk_shade_hits and their hooks): one kernel per
// family on the tree view of the first-hit buffers (query_view), on the scene's device (devices[0] of a multi-device scene), with events
// and a staging buffer of their own: nothing that describes vk_render's last frame is read or written.  What the families share is
// here: the argument checks of a batch (check_batch_args) and the host-pointer calls' chunked loop (run_batch).  A family adds its
// checks, its enqueue_* — device pointers and a stream, so that a device-pointer variant is a wrapper — and a BatchLayout.
namespace {

constexpr uint64_t RAY_CHUNK = 1ull << 20;      // rays staged at a time by the host variants (96 MiB of scratch for vk_trace_rays)

// The checks every batch call makes first.  what: the family's nouns for its parameter block ("trace") and its output ("hits").
struct BatchNouns { const char *params, *out; };
int check_batch_args(const vk_scene *scene, const void *params, uint32_t flags, uint64_t n, const void *in, const void *out,
    const BatchNouns &what) {
    if (!scene || !params) return fail(VK_ERR_BAD_ARG, std::string("null argument (scene or ") + what.params + " parameters)");
    if (flags != 0u) return fail(VK_ERR_BAD_ARG, std::string(what.params) + " flags must be 0");
    if (n > (1ull << 32)) return fail(VK_ERR_BAD_ARG, "n_rays exceeds 2^32");
    if (n != 0u && (!in || !out)) return fail(VK_ERR_BAD_ARG, std::string("null rays or ") + what.out + " with n_rays > 0");
    return VK_OK;
}

// One chunk's scratch in the scene's staging buffer: [head bytes][stream 0][stream 1]..., stream k holding `bytes` per ray for the `cap`
// rays of a chunk (the buffer may be larger than a call needs: every stream starts behind THIS call's earlier ones).  A stream with
// `in` is uploaded ahead of a chunk's launch, one with `out` downloaded behind it; one with neither is the kernels' own.
struct BatchStream {
    size_t bytes;
    const void *in;
    void *out;
};
struct BatchLayout {
    size_t head = 0;               // bytes ahead of the streams, cleared by the family's enqueue
    uint64_t cap = RAY_CHUNK;      // rays per chunk, at most
    int n_streams = 0;
    BatchStream stream[4] = {};
    size_t clamped_at = 0;         // != 0: a u64 at this offset of the head, read back per chunk and summed into vk_stats.clamped_samples
    uint64_t samples_per_ray = 1;  // vk_stats.samples = rays x this
};

// The host-pointer call of every family, its arguments checked and its device current: rays [0, n_rays) in chunks of L.cap through the
// staging buffer, each chunk uploaded, enqueued on the null stream between the scene's two ray-query events — enqueue(first_index,
// n, d_head, d_stream, stream) — waited for, timed and downloaded; then the stats.
template <class Enqueue>
int run_batch(vk_scene *q, BatchLayout L, uint64_t n_rays, uint64_t first_index, std::chrono::steady_clock::time_point t0,
    vk_stats *stats_out, Enqueue &&enqueue) {
    int rc;
    const uint64_t cap = n_rays < L.cap ? n_rays : L.cap;
    size_t per_ray = 0;
    for (int k = 0; k < L.n_streams; k++) per_ray += L.stream[k].bytes;
    if ((rc = q->rays.buf.ensure(L.head + (size_t)cap * per_ray)) != VK_OK) return rc;
    if ((rc = q->rays.ev0.create()) != VK_OK || (rc = q->rays.ev1.create()) != VK_OK) return rc;
    uint8_t *d_head = q->rays.buf, *d[4] = {nullptr, nullptr, nullptr, nullptr};
    {
        uint8_t *at = d_head + L.head;
        for (int k = 0; k < L.n_streams; k++) { d[k] = at; at += (size_t)cap * L.stream[k].bytes; }
    }
    double ms_sum = 0.0;
    uint64_t launches = 0, clamped = 0;
    for (uint64_t at = 0; at < n_rays; at += cap) {
        const uint64_t n = n_rays - at < cap ? n_rays - at : cap;
        for (int k = 0; k < L.n_streams; k++) {
            const BatchStream &s = L.stream[k];
            if (s.in) HIP_TRY(hipMemcpy(d[k], static_cast<const uint8_t *>(s.in) + at * s.bytes, (size_t)n * s.bytes, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipEventRecord(q->rays.ev0, nullptr));
        if ((rc = enqueue(first_index + at, n, d_head, d, (hipStream_t) nullptr)) != VK_OK) return rc;
        HIP_TRY(hipEventRecord(q->rays.ev1, nullptr));
        HIP_TRY(hipEventSynchronize(q->rays.ev1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, q->rays.ev0, q->rays.ev1));
        ms_sum += (double)ms; launches++;
        for (int k = 0; k < L.n_streams; k++) {
            const BatchStream &s = L.stream[k];
            if (s.out) HIP_TRY(hipMemcpy(static_cast<uint8_t *>(s.out) + at * s.bytes, d[k], (size_t)n * s.bytes, hipMemcpyDeviceToHost));
        }
        if (L.clamped_at) {
            unsigned long long c = 0;
            HIP_TRY(hipMemcpy(&c, d_head + L.clamped_at, sizeof(c), hipMemcpyDeviceToHost));
            clamped += c;
        }
    }
    if (stats_out) {
        stats_out->samples = n_rays * L.samples_per_ray; stats_out->kernel_ms = ms_sum; stats_out->kernel_launches = (uint32_t)launches;
        stats_out->clamped_samples = clamped;
        stats_out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return VK_OK;
}

// ---- closest hits (vk_trace_rays): trace_rays_kernel; the staging buffer holds rays, then hits
int check_trace_args(vk_scene *scene, const vk_trace_params *tp, const void *rays, uint64_t n_rays, const void *hits) {
    return check_batch_args(scene, tp, tp ? tp->flags : 0u, n_rays, rays, hits, {"trace", "hits"});
}

// the provenance tables, on the device with the scene's first ray query (freed with the scene's other uploads)
int ensure_provenance(vk_scene *q) {
    if (q->rays.prov_ready) return VK_OK;
    const LinearScene &H = *q->host;
    int rc;
    if ((rc = upload(q, H.src_sphere, q->rays.prov.sphere)) != VK_OK) return rc;
    if ((rc = upload(q, H.src_moving, q->rays.prov.moving)) != VK_OK) return rc;
    if ((rc = upload(q, H.src_rect, q->rays.prov.rect)) != VK_OK) return rc;
    if ((rc = upload(q, H.src_box_face, q->rays.prov.box_face)) != VK_OK) return rc;
    if ((rc = upload(q, H.src_medium, q->rays.prov.medium)) != VK_OK) return rc;
    q->rays.prov_ready = true;
    return VK_OK;
}

// one launch for rays [0, n) of d_rays, whose first ray is ray `first_index` of the caller's batch
int enqueue_trace(vk_scene *q, const vk_trace_params *tp, uint64_t first_index, const void *d_rays, uint64_t n, void *d_hits, hipStream_t st) {
    TraceArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "a ray query", &A.S);
    if (rc != VK_OK) return rc;
    A.P = q->rays.prov;
    A.rays = static_cast<const float4 *>(d_rays); A.hits = static_cast<uint4 *>(d_hits);
    A.seed = tp->seed; A.first_index = first_index; A.n_rays = n;
    const dim3 grid((uint32_t)((n + AOV_BLOCK - 1) / AOV_BLOCK));
    with_walk_variant(q->host->features, [&](auto f) {
        hipLaunchKernelGGL(trace_rays_kernel<decltype(f)::value>, grid, dim3(AOV_BLOCK), 0, st, A);
    });
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_trace_rays(vk_scene *scene, const vk_trace_params *params, const vk_ray *rays, uint64_t n_rays, vk_hit *hits, vk_stats *stats_out) {
    return guarded([&]() -> int {
        int rc = check_trace_args(scene, params, rays, n_rays, hits);
        if (rc != VK_OK) return rc;
        if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
        if (n_rays == 0u) return VK_OK;
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        BatchLayout L;
        L.n_streams = 2; L.stream[0] = {sizeof(vk_ray), rays, nullptr}; L.stream[1] = {sizeof(vk_hit), nullptr, hits};
        return run_batch(q, L, n_rays, params->first_index, t0, stats_out,
            [&](uint64_t first_index, uint64_t n, uint8_t *, uint8_t *const d[4], hipStream_t st) {
                return enqueue_trace(q, params, first_index, d[0], n, d[1], st);
            });
    });
}

int vk_trace_rays_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_hits, void *hip_stream,
    vk_stats *stats_out) {
    return guarded([&]() -> int {
        int rc = check_trace_args(scene, params, d_rays, n_rays, d_hits);
        if (rc != VK_OK) return rc;
        if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
        if (n_rays == 0u) return VK_OK;
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        if ((rc = enqueue_trace(q, params, params->first_index, d_rays, n_rays, d_hits, reinterpret_cast<hipStream_t>(hip_stream))) != VK_OK)
            return rc;
        if (stats_out) { stats_out->samples = n_rays; stats_out->kernel_launches = 1u; }
        return VK_OK;
    });
}

}  // extern "C"

// ---- ID mattes (vk_render_mattes): one launch of matte_kernel (vk_matte.hip) on the scene's device (devices[0] of a multi-device scene),
// on events and a staging buffer of the call's own; vk_matte_merge and vk_matte_mask are host code on the table's own insert and sort
// (vk_matte.h).  The provenance tables are the ray queries' (ensure_provenance).
namespace {

int check_matte_table(uint32_t ranks) {
    if (ranks < 1u || ranks > VK_MATTE_MAX_RANKS) return fail(VK_ERR_BAD_ARG, "matte ranks must be in 1..8");
    return VK_OK;
}

// vk_render_mattes' own checks, made first (they need no scene), then vk_render's; ids may be the hook's only array (counts_needed false)
int check_matte_args(vk_scene *scene, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, uint32_t kind,
    const void *ids, const void *counts, bool counts_needed) {
    if (!ids || (counts_needed && !counts)) return fail(VK_ERR_BAD_ARG, "null matte ids or counts");
    if (kind > (uint32_t)VK_MATTE_MATERIAL) return fail(VK_ERR_BAD_ARG, "unknown matte kind");
    int rc = check_call_args(scene, cam, p);
    if (rc != VK_OK) return rc;
    if ((uint64_t)first_sample + p->samples_per_pixel > 0xFFFFFFFFull) return fail(VK_ERR_BAD_ARG,
        "first_sample + samples_per_pixel exceeds 2^32 - 1");
    return VK_OK;
}

// the kernels' arguments without their arrays; the provenance tables are on the device afterwards
int matte_args(vk_scene *q, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, uint32_t kind, uint32_t ranks,
    const TileGeom &g, MatteArgs *A) {
    memset(A, 0, sizeof(*A));
    int rc = query_view(q, "the matte walk", &A->S);
    if (rc != VK_OK) return rc;
    if ((rc = ensure_provenance(q)) != VK_OK) return rc;
    A->P = q->rays.prov;
    A->C.cam = *cam;
    A->C.width = p->width; A->C.height = p->height; A->C.spp = p->samples_per_pixel; A->C.seed = p->seed;
    A->kind = kind; A->ranks = ranks;
    A->first_sample = first_sample; A->tiles_x = g.tiles_x; A->tile_rank = g.rank; A->tile_world = g.world; A->n_local = g.n_local;
    return VK_OK;
}

size_t round16(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }

// folds (id, c) pairs and overflow of table b's pixel into a's, in b's order, and sorts again (vk_matte_merge; vk_matte.h's rule)
void matte_merge_pixel(uint32_t ranks, uint32_t *ids, uint32_t *counts, uint32_t *overflow, const uint32_t *ids_b, const uint32_t *counts_b,
    const uint32_t *overflow_b) {
    MatteTable T;
    matte_clear(T);
    for (uint32_t r = 0; r < ranks && counts[r] != 0u; r++) { T.id[r] = ids[r]; T.cnt[r] = counts[r]; T.used = r + 1u; }
    for (uint32_t r = 0; r < ranks && counts_b[r] != 0u; r++) matte_insert(T, ranks, ids_b[r], counts_b[r]);
    matte_sort(T);
    for (uint32_t r = 0; r < ranks; r++) { ids[r] = T.id[r]; counts[r] = T.cnt[r]; }
    if (overflow) *overflow += T.overflow + *overflow_b;
}

}  // namespace

extern "C" {

int vk_matte_default_params(vk_matte_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null matte parameters");
    out->kind = VK_MATTE_OBJECT; out->ranks = 6u; out->flags = 0u; out->_pad = 0u;
    return VK_OK;
}

int vk_render_mattes(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample, const vk_matte_params *mp,
    uint32_t *ids, uint32_t *counts, uint32_t *overflow, vk_stats *stats_out) {
    return guarded([&]() -> int {
        if (!mp) return fail(VK_ERR_BAD_ARG, "null matte parameters");
        int rc = check_matte_table(mp->ranks);
        if (rc != VK_OK) return rc;
        if (mp->flags != 0u) return fail(VK_ERR_BAD_ARG, "matte flags must be 0");
        if ((rc = check_matte_args(scene, cam, params, first_sample, mp->kind, ids, counts, true)) != VK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        const TileGeom g(params);
        MatteArgs A;
        if ((rc = matte_args(q, cam, params, first_sample, mp->kind, mp->ranks, g, &A)) != VK_OK) return rc;
        // ids, counts and overflow side by side in the call's own staging buffer, each slice 16-byte aligned
        const size_t n_pixels = (size_t)params->width * params->height;
        const size_t slots = n_pixels * mp->ranks * sizeof(uint32_t), per_pixel = n_pixels * sizeof(uint32_t);
        if ((rc = q->matte.buf.ensure(2u * round16(slots) + (overflow ? per_pixel : 0u))) != VK_OK) return rc;
        A.ids = reinterpret_cast<uint32_t *>(q->matte.buf.get());
        A.counts = reinterpret_cast<uint32_t *>(q->matte.buf.get() + round16(slots));
        A.overflow = overflow ? reinterpret_cast<uint32_t *>(q->matte.buf.get() + 2u * round16(slots)) : nullptr;
        // a partition: the caller's pixels outside it must come back untouched
        if (g.world > 1u) {
            HIP_TRY(hipMemcpy(A.ids, ids, slots, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(A.counts, counts, slots, hipMemcpyHostToDevice));
            if (overflow) HIP_TRY(hipMemcpy(A.overflow, overflow, per_pixel, hipMemcpyHostToDevice));
        }
        if ((rc = q->matte.ev0.create()) != VK_OK || (rc = q->matte.ev1.create()) != VK_OK) return rc;
        HIP_TRY(hipEventRecord(q->matte.ev0, nullptr));
        if (g.n_local != 0u) {
            launch_matte(q->host->features, A);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(q->matte.ev1, nullptr));
        HIP_TRY(hipMemcpy(ids, A.ids, slots, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts, A.counts, slots, hipMemcpyDeviceToHost));
        if (overflow) HIP_TRY(hipMemcpy(overflow, A.overflow, per_pixel, hipMemcpyDeviceToHost));
        if (stats_out) aov_stats(params, stats_out);
        return end_timed_call(q->matte.ev0, q->matte.ev1, t0, stats_out);
    });
}

int vk_matte_merge(uint32_t ranks, uint64_t n_pixels, uint32_t *ids, uint32_t *counts, uint32_t *overflow, const uint32_t *ids_b,
    const uint32_t *counts_b, const uint32_t *overflow_b) {
    int rc = check_matte_table(ranks);
    if (rc != VK_OK) return rc;
    if ((overflow != nullptr) != (overflow_b != nullptr)) return fail(VK_ERR_BAD_ARG, "matte overflow arrays: both or neither");
    if (n_pixels > 0u && (!ids || !counts || !ids_b || !counts_b)) return fail(VK_ERR_BAD_ARG, "null matte table");
    for (uint64_t i = 0; i < n_pixels; i++)
        matte_merge_pixel(ranks, ids + i * ranks, counts + i * ranks, overflow ? overflow + i : nullptr, ids_b + i * ranks,
                          counts_b + i * ranks, overflow_b ? overflow_b + i : nullptr);
    return VK_OK;
}

int vk_matte_mask(uint32_t ranks, uint64_t n_pixels, const uint32_t *ids, const uint32_t *counts, uint32_t n_samples, const uint32_t *want,
    uint32_t n_want, float *mask_out) {
    int rc = check_matte_table(ranks);
    if (rc != VK_OK) return rc;
    if (n_samples == 0u) return fail(VK_ERR_BAD_ARG, "matte mask: n_samples must be >= 1");
    if (!want && n_want > 0u) return fail(VK_ERR_BAD_ARG, "null matte id set");
    if (n_pixels > 0u && (!ids || !counts || !mask_out)) return fail(VK_ERR_BAD_ARG, "null matte table");
    for (uint64_t i = 0; i < n_pixels; i++) {
        uint32_t sum = 0u;
        for (uint32_t r = 0; r < ranks; r++) {
            if (counts[i * ranks + r] == 0u) continue;                // a free slot holds no id
            bool in = false;
            for (uint32_t w = 0; w < n_want && !in; w++) in = want[w] == ids[i * ranks + r];
            if (in) sum += counts[i * ranks + r];
        }
        mask_out[i] = (float)sum / (float)n_samples;
    }
    return VK_OK;
}

int vk_debug_matte_samples(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample, uint32_t kind,
    uint32_t *ids_out) {
    return guarded([&]() -> int {
        int rc = check_matte_args(scene, cam, params, first_sample, kind, ids_out, nullptr, false);
        if (rc != VK_OK) return rc;
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        const TileGeom g(params);
        MatteArgs A;
        if ((rc = matte_args(q, cam, params, first_sample, kind, 1u, g, &A)) != VK_OK) return rc;
        const size_t bytes = (size_t)params->width * params->height * params->samples_per_pixel * sizeof(uint32_t);
        if ((rc = q->matte.buf.ensure(bytes)) != VK_OK) return rc;
        A.ids = reinterpret_cast<uint32_t *>(q->matte.buf.get());
        if (g.world > 1u) HIP_TRY(hipMemcpy(A.ids, ids_out, bytes, hipMemcpyHostToDevice));
        if (g.n_local != 0u) {
            launch_matte_samples(q->host->features, A);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpy(ids_out, A.ids, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

}  // extern "C"

// ---- occlusion queries (vk_trace_occluded): occlusion_kernel; the staging buffer holds rays, then one byte per ray.  No provenance: the
// call names no object.
namespace {

int check_occlusion_args(vk_scene *scene, const vk_trace_params *tp, const void *rays, uint64_t n_rays, const void *occluded) {
    return check_batch_args(scene, tp, tp ? tp->flags : 0u, n_rays, rays, occluded, {"trace", "occluded"});
}

template <bool REFILL>
void launch_occlusion(uint32_t features, const OcclusionArgs &A, hipStream_t st) {
    // one ray per lane, or one block of 64 * k rays per wave
    const uint64_t per_group = REFILL ? 64ull * A.k * (AOV_BLOCK / 64) : (uint64_t)AOV_BLOCK;
    const dim3 grid((uint32_t)((A.n_rays + per_group - 1) / per_group));
    with_walk_variant(features, [&](auto f) {
        hipLaunchKernelGGL((occlusion_kernel<decltype(f)::value, REFILL>), grid, dim3(AOV_BLOCK), 0, st, A);
    });
}

// one launch for rays [0, n) of d_rays, whose first ray is ray `first_index` of the caller's batch
int enqueue_occlusion(vk_scene *q, const vk_trace_params *tp, uint64_t first_index, const void *d_rays, uint64_t n, void *d_occluded,
    hipStream_t st, bool refill = OCC_PRODUCTION_REFILL, uint32_t k = OCC_K, uint32_t t = OCC_T) {
    OcclusionArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "an occlusion query", &A.S);
    if (rc != VK_OK) return rc;
    A.rays = static_cast<const float4 *>(d_rays); A.occluded = static_cast<uint8_t *>(d_occluded);
    A.seed = tp->seed; A.first_index = first_index; A.n_rays = n;
    A.k = k; A.t = t;
#ifdef VK_DEBUG_LIB      // both forms (vk_debug_trace_occluded_device); the product library holds the production form only
    if (refill) launch_occlusion<true>(q->host->features, A, st); else launch_occlusion<false>(q->host->features, A, st);
#else
    if (refill != OCC_PRODUCTION_REFILL) return fail(VK_ERR_UNSUPPORTED, "this form of the occlusion kernel is in the debug library only");
    launch_occlusion<OCC_PRODUCTION_REFILL>(q->host->features, A, st);
#endif
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_trace_occluded(vk_scene *scene, const vk_trace_params *params, const vk_ray *rays, uint64_t n_rays, uint8_t *occluded,
    vk_stats *stats_out) {
    return guarded([&]() -> int {
        int rc = check_occlusion_args(scene, params, rays, n_rays, occluded);
        if (rc != VK_OK) return rc;
        if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
        if (n_rays == 0u) return VK_OK;
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        BatchLayout L;
        L.n_streams = 2; L.stream[0] = {sizeof(vk_ray), rays, nullptr}; L.stream[1] = {1u, nullptr, occluded};
        return run_batch(q, L, n_rays, params->first_index, t0, stats_out,
            [&](uint64_t first_index, uint64_t n, uint8_t *, uint8_t *const d[4], hipStream_t st) {
                return enqueue_occlusion(q, params, first_index, d[0], n, d[1], st);
            });
    });
}

int vk_trace_occluded_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_occluded,
    void *hip_stream, vk_stats *stats_out) {
    return guarded([&]() -> int {
        int rc = check_occlusion_args(scene, params, d_rays, n_rays, d_occluded);
        if (rc != VK_OK) return rc;
        if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
        if (n_rays == 0u) return VK_OK;
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = enqueue_occlusion(q, params, params->first_index, d_rays, n_rays, d_occluded, reinterpret_cast<hipStream_t>(hip_stream))) != VK_OK)
            return rc;
        if (stats_out) { stats_out->samples = n_rays; stats_out->kernel_launches = 1u; }
        return VK_OK;
    });
}

// test and report hook: vk_trace_occluded_device through the named form of the kernel (vecchio_amd_debug.h; the product library holds
// the production form only and refuses the other one)
int vk_debug_trace_occluded_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_occluded,
    void *hip_stream, int refill, uint32_t k, uint32_t t) {
    return guarded([&]() -> int {
        int rc = check_occlusion_args(scene, params, d_rays, n_rays, d_occluded);
        if (rc != VK_OK) return rc;
        if (refill != 0 && (k < 1u || k > 4096u || t < 1u || t > 64u)) return fail(VK_ERR_BAD_ARG, "k must be in 1..4096 and t in 1..64");
        if (n_rays == 0u) return VK_OK;
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        return enqueue_occlusion(q, params, params->first_index, d_rays, n_rays, d_occluded, reinterpret_cast<hipStream_t>(hip_stream),
                                 refill != 0, k, t);
    });
}

}  // extern "C"

// ---- radiance queries (vk_trace_radiance): radiance_kernel.  The scratch of one chunk: [unit counter, clamped count: 32 bytes][rays]
// [fixed-point sums][means] — or, for the per-sample hook, [32 bytes][rays][samples][keys].
// Irradiance queries (vk_trace_irradiance) are the same calls with `gather` set: gather_kernel instead of radiance_kernel, the rays read
// as (point, normal) records, no keys, and in the hook's scratch the drawn directions where the keys would be.
// Probe queries (vk_trace_probes) are the same calls with mode QM_PROBE: probe_kernel, the rays read as probes (the direction not read),
// 27 fixed-point sums and 27 means a probe instead of 3, and the hook's scratch as the irradiance hook's.
namespace {

static_assert(sizeof(RadianceKey) == sizeof(vk_debug_stream_key) && sizeof(RadianceKey) == 24, "vk_debug_stream_key is what the kernel reads");
constexpr size_t RAD_HEAD = 32;                  // bytes ahead of the rays: unit counter (u32), pad, clamped samples (u64), pad
constexpr uint64_t RAD_HOOK_SAMPLES = 1ull << 22;    // samples per launch of the per-sample hook (64 MiB of them)

int check_radiance_args(vk_scene *scene, const vk_radiance_params *rp, const void *rays, uint64_t n_rays, const void *out) {
    int rc = check_batch_args(scene, rp, rp ? rp->flags : 0u, n_rays, rays, out, {"radiance", "output"});
    if (rc != VK_OK) return rc;
    if (rp->samples_per_ray == 0u || rp->samples_per_ray > (1u << 26)) return fail(VK_ERR_BAD_ARG, "samples_per_ray must be in 1..2^26");
    if ((uint64_t)rp->first_sample + rp->samples_per_ray > 0xFFFFFFFFull) return fail(VK_ERR_BAD_ARG,
        "first_sample + samples_per_ray exceeds 2^32 - 1");
    if (rp->integrator > VK_INTEGRATOR_SCATTER || rp->background > VK_BACKGROUND_SKY) return fail(VK_ERR_BAD_ARG, "bad integrator/background");
    return VK_OK;
}

template <uint32_t F, int MODE>
int launch_radiance(const RadianceArgs &A, dim3 grid, hipStream_t st) {
    // Six waves per SIMD (80 VGPRs), as render_kernel's variants — except the everything-variants: render_kernel calls their SHADE + REFILL
    // phase out of line to hold them there (shade_refill_call); this kernel keeps its phase inline, where 80 registers cost them ~500
    // scratch instructions, so they are built for four (128 VGPRs)
    constexpr int MINW = (F & VKF_ALL_SCENE) == VKF_ALL_SCENE ? 4 : 6;
    // (gather_kernel, probe_kernel: the same rule; DESIGN.md "Irradiance queries" and "Probe queries" have their instances' numbers)
    auto kernel = MODE == QM_PROBE ? &probe_kernel<F, MINW> : (MODE == QM_GATHER ? &gather_kernel<F, MINW> : &radiance_kernel<F, MINW>);
    const size_t shmem = (size_t)(RAD_BLOCK / 64) * query_block_floats<F, MODE>() * sizeof(float);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(kernel, grid, dim3(RAD_BLOCK), shmem, st, A);
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

// one launch for rays [0, n) of d_rays, whose first ray is ray `first_index` of the caller's batch: means into d_rgb through d_accum, or
// (d_samples != null) every sample into d_samples.  d_head: RAD_HEAD bytes (cleared here).  QM_GATHER: d_rays holds points, gather_kernel
// runs, and with d_samples every sample's direction goes to d_dirs where that is given.  QM_PROBE: d_rays holds probes, probe_kernel
// runs, d_accum and d_rgb hold 27 values a probe, d_dirs as for QM_GATHER.
int enqueue_radiance(vk_scene *q, const vk_radiance_params *rp, uint64_t first_index, const void *d_rays, const void *d_keys, uint32_t n,
    uint8_t *d_head, long long *d_accum, float *d_rgb, float *d_samples, hipStream_t st, int mode = QM_RAY, float *d_dirs = nullptr) {
    RadianceArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "a radiance query", &A.S);
    if (rc != VK_OK) return rc;
    A.C.spp = rp->samples_per_ray; A.C.max_depth = rp->max_depth; A.C.seed = rp->seed;
    A.C.integrator = rp->integrator; A.C.background = rp->background;
    A.C.bg[0] = rp->background_color[0]; A.C.bg[1] = rp->background_color[1]; A.C.bg[2] = rp->background_color[2];
    A.rays = static_cast<const float4 *>(d_rays); A.keys = static_cast<const RadianceKey *>(d_keys);
    A.accum = d_samples ? nullptr : d_accum; A.samples = reinterpret_cast<float4 *>(d_samples);
    A.dirs = mode != QM_RAY && d_samples ? reinterpret_cast<float4 *>(d_dirs) : nullptr;
    A.counter = reinterpret_cast<uint32_t *>(d_head); A.clamped = reinterpret_cast<unsigned long long *>(d_head + 8);
    A.accum_clamp = accum_clamp_for(rp->samples_per_ray);
    A.first_index = first_index; A.n_rays = n; A.first_sample = rp->first_sample;
    A.shade_defer = SHADE_DEFER; A.prim_weight = q->plan.hot_bytes > (4u << 20) ? 3u : 1u;
    // Units: (64 rays, a chunk of samples) — probe_kernel: (8 probes, a chunk of samples).  Enough of them to keep every wave of the launch busy four times over where the samples
    // allow it, at least four samples to a chunk; a chunk stays below 2^16 samples (the kernel counts 64 x that in 32 bits).  Any choice
    // gives the same sums.
    const uint32_t slots = mode == QM_PROBE ? PROBE_SLOTS : 64u, values = mode == QM_PROBE ? PROBE_VALUES : 3u;
    const uint32_t spp = rp->samples_per_ray, n_blocks = (n + slots - 1u) / slots;
    const uint32_t waves = (uint32_t)q->num_cus * 24u;
    uint32_t n_chunks = (4u * waves + n_blocks - 1u) / n_blocks;
    const uint32_t hi = spp / 4u > 4096u ? 4096u : (spp / 4u ? spp / 4u : 1u), lo = (spp + 65535u) / 65536u;
    if (n_chunks > hi) n_chunks = hi;
    if (n_chunks < lo) n_chunks = lo;
    A.n_chunks = n_chunks;
    const uint64_t units = (uint64_t)n_blocks * n_chunks;        // <= 2^14 * 2^12 (probes: 2^17 * 2^12) for the host calls' chunks of 2^20 rays
    if (units >= (1ull << 31)) return fail(VK_ERR_BAD_ARG, "internal error: too many work units in one radiance launch");
    const uint64_t groups = (units + (RAD_BLOCK / 64) - 1) / (RAD_BLOCK / 64), full = (uint64_t)q->num_cus * 6u;   // (24 waves per CU)
    const dim3 grid((uint32_t)(groups < full ? groups : full));
    HIP_TRY(hipMemsetAsync(d_head, 0, RAD_HEAD, st));
    if (A.accum) HIP_TRY(hipMemsetAsync(d_accum, 0, (size_t)n * values * sizeof(long long), st));
    const uint32_t F = pick_variant(q) | (rp->integrator == VK_INTEGRATOR_PDF ? (uint32_t)VKF_INTEG_PDF : 0u);
    rc = with_variant(F, [&](auto f) {
        constexpr uint32_t FV = decltype(f)::value;
        return mode == QM_PROBE ? launch_radiance<FV, QM_PROBE>(A, grid, st)
             : (mode == QM_GATHER ? launch_radiance<FV, QM_GATHER>(A, grid, st) : launch_radiance<FV, QM_RAY>(A, grid, st));
    });
    if (rc != VK_OK) return rc;
    if (A.accum) {
        const uint32_t nv = n * values;          // (n <= 2^20 from the host calls)
        hipLaunchKernelGGL(radiance_resolve_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, st, d_accum, d_rgb, nv, spp);
        HIP_TRY(hipGetLastError());
    }
    return VK_OK;
}

// the host call behind vk_trace_radiance (keys == null, samples_out == null) and its per-sample hook; with QM_GATHER the one behind
// vk_trace_irradiance and its hook (rays = the points, keys == null; dirs_out: the hook's directions, or null); with QM_PROBE the one
// behind vk_trace_probes and its hook (rays = the probes, rgb_out = sh_out: 27 floats a probe)
int radiance_host(vk_scene *scene, const vk_radiance_params *rp, const vk_ray *rays, uint64_t n_rays, const vk_debug_stream_key *keys,
    float *rgb_out, float *samples_out, vk_stats *stats_out, int mode = QM_RAY, float *dirs_out = nullptr) {
    int rc = check_radiance_args(scene, rp, rays, n_rays, samples_out ? samples_out : rgb_out);
    if (rc != VK_OK) return rc;
    if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
    if (n_rays == 0u) return VK_OK;
    // (the handle is read from here on)
    if ((rc = check_integrator_for_scene(*scene->host, rp->integrator)) != VK_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t spp = rp->samples_per_ray;
    const size_t values = mode == QM_PROBE ? PROBE_VALUES : 3u;      // per ray: fixed-point sums, and means
    if (rp->max_depth == 0u) {        // every sample is (0,0,0) (main.rs:126-128) and draws nothing
        if (samples_out) {
            for (uint64_t i = 0; i < n_rays; i++) for (uint32_t k = 0; k < spp; k++) {
                float *o = samples_out + (i * spp + k) * 4u;
                const uint32_t ctr = keys ? keys[i].ctr : 0u;
                o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; memcpy(o + 3, &ctr, 4);
            }
            if (dirs_out) memset(dirs_out, 0, (size_t)n_rays * spp * 16u);          // (no direction is drawn either)
        } else {
            memset(rgb_out, 0, (size_t)n_rays * values * sizeof(float));
        }
        if (stats_out) stats_out->samples = n_rays * spp;
        return VK_OK;
    }
    vk_scene *q = first_part(scene);
    HIP_TRY(hipSetDevice(q->device));
    BatchLayout L;
    L.head = RAD_HEAD; L.clamped_at = 8; L.samples_per_ray = spp; L.n_streams = 3;
    L.stream[0] = {sizeof(vk_ray), rays, nullptr};
    if (samples_out) {      // the hook: samples, then keys (uploaded where given) or the directions
        const uint64_t c = RAD_HOOK_SAMPLES / spp ? RAD_HOOK_SAMPLES / spp : 1u;
        if (L.cap > c) L.cap = c;
        L.stream[1] = {(size_t)spp * 16u, nullptr, samples_out};
        if (dirs_out) L.stream[2] = {(size_t)spp * 16u, nullptr, dirs_out};
        else L.stream[2] = {sizeof(vk_debug_stream_key), keys, nullptr};
    } else {                // means: the fixed-point sums, then the means
        L.stream[1] = {values * sizeof(long long), nullptr, nullptr};
        L.stream[2] = {values * sizeof(float), nullptr, rgb_out};
    }
    return run_batch(q, L, n_rays, rp->first_index, t0, stats_out,
        [&](uint64_t first_index, uint64_t n, uint8_t *d_head, uint8_t *const d[4], hipStream_t st) {
            if (samples_out) return enqueue_radiance(q, rp, first_index, d[0], keys ? d[2] : nullptr, (uint32_t)n, d_head, nullptr, nullptr,
                                                     reinterpret_cast<float *>(d[1]), st, mode,
                                                     dirs_out ? reinterpret_cast<float *>(d[2]) : nullptr);
            return enqueue_radiance(q, rp, first_index, d[0], nullptr, (uint32_t)n, d_head, reinterpret_cast<long long *>(d[1]),
                                    reinterpret_cast<float *>(d[2]), nullptr, st, mode);
        });
}

}  // namespace

extern "C" {

int vk_trace_radiance(vk_scene *scene, const vk_radiance_params *params, const vk_ray *rays, uint64_t n_rays, float *rgb_out,
    vk_stats *stats_out) {
    return guarded([&]() -> int { return radiance_host(scene, params, rays, n_rays, nullptr, rgb_out, nullptr, stats_out); });
}

// test hook (vecchio_amd_debug.h): every sample of the query, optionally on streams resumed from keys
int vk_debug_trace_radiance_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *rays, uint64_t n_rays,
    const vk_debug_stream_key *keys, float *samples_out, vk_stats *stats_out) {
    return guarded([&]() -> int {
        if (n_rays != 0u && !samples_out) return fail(VK_ERR_BAD_ARG, "null samples buffer");
        return radiance_host(scene, params, rays, n_rays, keys, nullptr, samples_out, stats_out);
    });
}

int vk_trace_irradiance(vk_scene *scene, const vk_radiance_params *params, const vk_ray *points, uint64_t n_points, float *rgb_out,
    vk_stats *stats_out) {
    return guarded([&]() -> int { return radiance_host(scene, params, points, n_points, nullptr, rgb_out, nullptr, stats_out, QM_GATHER); });
}

// test hook (vecchio_amd_debug.h): every sample of the query and, where asked for, the direction drawn for it
int vk_debug_trace_irradiance_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *points, uint64_t n_points,
    float *samples_out, float *dirs_out, vk_stats *stats_out) {
    return guarded([&]() -> int {
        if (n_points != 0u && !samples_out) return fail(VK_ERR_BAD_ARG, "null samples buffer");
        return radiance_host(scene, params, points, n_points, nullptr, nullptr, samples_out, stats_out, QM_GATHER, dirs_out);
    });
}

int vk_trace_probes(vk_scene *scene, const vk_radiance_params *params, const vk_ray *probes, uint64_t n_probes, float *sh_out,
    vk_stats *stats_out) {
    return guarded([&]() -> int { return radiance_host(scene, params, probes, n_probes, nullptr, sh_out, nullptr, stats_out, QM_PROBE); });
}

// test hook (vecchio_amd_debug.h): every sample of the query and, where asked for, the direction drawn for it
int vk_debug_trace_probe_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *probes, uint64_t n_probes,
    float *samples_out, float *dirs_out, vk_stats *stats_out) {
    return guarded([&]() -> int {
        if (n_probes != 0u && !samples_out) return fail(VK_ERR_BAD_ARG, "null samples buffer");
        return radiance_host(scene, params, probes, n_probes, nullptr, nullptr, samples_out, stats_out, QM_PROBE, dirs_out);
    });
}

// rgb[c] = sum_k w_l(k) * sh[k * 3 + c] * Y_k(unit(n)) in double, rounded once (plain host code: no device, no handle)
int vk_probe_eval(const float *sh27, const float n[3], uint32_t mode, float rgb[3]) {
    return guarded([&]() -> int {
        if (!sh27 || !n || !rgb) return fail(VK_ERR_BAD_ARG, "null argument (sh27, n or rgb)");
        if (mode > 1u) return fail(VK_ERR_BAD_ARG, "mode must be 0 (radiance) or 1 (irradiance / pi)");
        const double len = std::sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
        const double x = n[0] / len, y = n[1] / len, z = n[2] / len;
        const double Y[9] = {0.282095, 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z),
                             0.315392 * (3.0 * (z * z) - 1.0), 1.092548 * (x * z), 0.546274 * (x * x - y * y)};
        const double pi = 3.14159265358979323846;
        for (int c = 0; c < 3; c++) {
            double v = 0.0;
            for (int k = 0; k < 9; k++) {
                const double w = mode == 0u ? 4.0 * pi : (k == 0 ? 4.0 * pi : (k < 4 ? 8.0 * pi / 3.0 : pi));
                v += w * (double)sh27[k * 3 + c] * Y[k];
            }
            rgb[c] = (float)v;
        }
        return VK_OK;
    });
}

}  // extern "C"

// ---- shade queries (vk_shade_hits): shade_hits_kernel.  The scratch of one chunk: [rays][hits][states][results], 240 bytes an item.
namespace {

constexpr uint64_t SHADE_CHUNK = 1ull << 19;     // items staged at a time (120 MiB of scratch: vk_trace_rays' chunk takes 96)
static_assert(sizeof(vk_path_state) == 48 && sizeof(vk_shaded) == 96, "what shade_hits_kernel reads and writes");

// the call's parameters as the radiance family's, for its checks (one sample, nothing of a batch's indices)
vk_radiance_params shade_as_radiance(const vk_shade_params *sp) {
    vk_radiance_params rp;
    memset(&rp, 0, sizeof(rp));
    rp.samples_per_ray = 1u; rp.max_depth = sp->max_depth; rp.integrator = sp->integrator; rp.background = sp->background;
    rp.background_color[0] = sp->background_color[0]; rp.background_color[1] = sp->background_color[1];
    rp.background_color[2] = sp->background_color[2];
    rp.flags = sp->flags;
    return rp;
}

// one launch for items [0, n) of d_rays, d_hits and d_states
int enqueue_shade(vk_scene *q, const vk_shade_params *sp, const void *d_rays, const void *d_hits, const void *d_states, uint64_t n,
    void *d_out, hipStream_t st) {
    ShadeArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "a shade query", &A.S);
    if (rc != VK_OK) return rc;
    A.C.spp = 1u; A.C.max_depth = sp->max_depth; A.C.integrator = sp->integrator; A.C.background = sp->background;
    A.C.bg[0] = sp->background_color[0]; A.C.bg[1] = sp->background_color[1]; A.C.bg[2] = sp->background_color[2];
    A.rays = static_cast<const float4 *>(d_rays); A.hits = static_cast<const uint4 *>(d_hits);
    A.states = static_cast<const uint4 *>(d_states); A.out = static_cast<uint4 *>(d_out);
    A.n = n; A.n_materials = (uint32_t)q->host->materials.size();
    const dim3 grid((uint32_t)((n + AOV_BLOCK - 1) / AOV_BLOCK));
    // every scene feature, whatever the scene has: with_variant's last two cases
    with_variant(VKF_ALL_SCENE | (sp->integrator == VK_INTEGRATOR_PDF ? (uint32_t)VKF_INTEG_PDF : 0u), [&](auto f) {
        constexpr uint32_t FV = decltype(f)::value;
        if constexpr ((FV & VKF_ALL_SCENE) == VKF_ALL_SCENE) hipLaunchKernelGGL(shade_hits_kernel<FV>, grid, dim3(AOV_BLOCK), 0, st, A);
    });
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_shade_hits(vk_scene *scene, const vk_shade_params *params, const vk_ray *rays, const vk_hit *hits, const vk_path_state *states,
    uint64_t n, vk_shaded *out, vk_stats *stats_out) {
    return guarded([&]() -> int {
        const void *in = rays && hits && states ? static_cast<const void *>(rays) : nullptr;
        int rc = check_batch_args(scene, params, params ? params->flags : 0u, n, in, out, {"shade", "shaded"});
        if (rc != VK_OK) return rc;
        const vk_radiance_params rp = shade_as_radiance(params);
        if ((rc = check_radiance_args(scene, &rp, in, n, out)) != VK_OK) return rc;
        if (stats_out) memset(stats_out, 0, sizeof(*stats_out));
        if (n == 0u) return VK_OK;
        // (the handle is read from here on)
        if ((rc = check_integrator_for_scene(*scene->host, params->integrator)) != VK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        BatchLayout L;
        L.cap = SHADE_CHUNK; L.n_streams = 4;
        L.stream[0] = {sizeof(vk_ray), rays, nullptr}; L.stream[1] = {sizeof(vk_hit), hits, nullptr};
        L.stream[2] = {sizeof(vk_path_state), states, nullptr}; L.stream[3] = {sizeof(vk_shaded), nullptr, out};
        return run_batch(q, L, n, 0u, t0, stats_out,
            [&](uint64_t, uint64_t m, uint8_t *, uint8_t *const d[4], hipStream_t st) {
                return enqueue_shade(q, params, d[0], d[1], d[2], m, d[3], st);
            });
    });
}

}  // extern "C"

// ---- path batches (vk_paths_*): trace_paths_kernel, shade_hits_kernel (enqueue_shade, unchanged) and the compaction's three launches
// per bounce, on the null stream, on buffers and events the handle owns: nothing of the scene handle is written but its provenance
// tables (ensure_provenance), and nothing that describes vk_render's last frame or the ray queries' scratch is touched.
struct vk_paths {
    vk_scene *scene = nullptr;                      // as handed to vk_paths_create
    uint64_t capacity = 0;
    DeviceBuffer<uint8_t> rays, states, hits, shaded, result_state;      // vk_ray, vk_path_state, vk_hit, vk_shaded, vk_path_state [capacity]
    DeviceBuffer<uint32_t> ids[2], result_status;   // the live paths' ids, double-buffered (the compaction is never in place); [capacity]
    DeviceBuffer<uint32_t> wg_counts, wg_offsets;   // the compaction's tables: [5][n_wg], [n_wg]
    DeviceBuffer<unsigned long long> counts;        // [5]: the one record a bounce sends back
    Event ev0, ev1;                                 // around a bounce's launches
    Event ev_t, ev_s;                               // behind its trace and behind its shade (vk_debug_paths_last_ms)
    Event ev_e;                                     // behind a regenerating bounce's top-up (vk_debug_regen_last_ms)
    vk_shade_params sp{};                           // the last begin's
    bool begun = false;
    bool deposited = false;                         // vk_film_deposit has taken this batch (cleared by vk_paths_begin and vk_film_emit)
    bool splatted = false;                          // vk_splat_deposit has taken this batch (cleared where `deposited` is)
    bool bucketed = false;                          // vk_robust_deposit has taken this batch (cleared where `deposited` is)
    bool layered = false;                           // vk_lpe_deposit has taken this batch (cleared where `deposited` is)
    uint64_t begins = 0;                            // host only: the begins, emits and regen begins so far (a vk_lpe tracker binds to one)
    uint32_t cur = 0;                               // ids[cur] holds the live ids
    uint64_t started = 0, live = 0, retired[5] = {0, 0, 0, 0, 0};
    uint32_t bounces = 0;
    // the regenerating state (vk_regen_*), host side only: set by vk_regen_begin, cleared by vk_paths_begin and vk_film_emit
    bool regen = false;
    const vk_film *regen_film = nullptr;            // the run's film, for the identity check only: never dereferenced
    vk_film_window regen_win{};
    uint64_t regen_next = 0, regen_total = 0;       // the window's paths [0, regen_next) are emitted, of regen_total
    // a tile run (vk_adapt_begin): the window is the film's active tiles, samples [regen_first_sample, + regen_n_samples); regen_win unused
    bool regen_tiles = false;
    uint32_t regen_first_sample = 0, regen_n_samples = 0;
    // the termination rule (vk_roulette_set): the handle's, not a batch's — no begin, emit or reset touches it
    bool roulette = false;
    vk_roulette_params rr{};
};
// a film's error moments and tile map (vk_adapt_*, below): allocated by vk_adapt_enable, on the film's device
struct AdaptState {
    bool judged = false;                            // parameters given: the rule runs behind every close
    vk_adaptive_params ap{};
    DeviceBuffer<long long> prev;                   // the sums at the last close, [width * height * 3]
    DeviceBuffer<double> m2;                        // sum_j n_j m_j^2, [width * height * 3]
    DeviceBuffer<uint32_t> tile_n, tile_k;          // [tiles]: 0 = active, else the count and the closes the tile froze with
    DeviceBuffer<uint32_t> list, prefix;            // [tiles], [tiles + 1]: the active tiles, ascending, and the pixels before each
    DeviceBuffer<uint32_t> block_tiles, block_px;   // the rebuild's tables, [ceil(tiles / 1024)]
    DeviceBuffer<unsigned long long> record;        // [2]: the one record a close sends back — active tiles, their pixels
    uint32_t tiles_x = 0, tiles = 0;
    uint32_t done = 0, steps = 0;                   // samples_done, steps
    uint32_t n_active = 0;                          // as of the last rebuild
    uint64_t px_active = 0, samples_rendered = 0;   // the active tiles' in-image pixels; pixel-samples the closes have counted
};
// a film (vk_film_*, below): here because a regenerating batch's compaction deposits into one
struct vk_film {
    vk_scene *scene = nullptr;                      // as handed to vk_film_create
    vk_camera cam;
    vk_render_params params;
    DeviceBuffer<unsigned long long> sums;          // [width * height * 3], two's complement
    DeviceBuffer<unsigned long long> counters;      // the counter record: deposited, dropped, clamped, skipped
    DeviceBuffer<float> out;                        // the resolved frame on its way to the host (allocated by the first vk_film_resolve)
    Event ev[6];                                    // around the last emit, deposit and resolve
    bool timed[3] = {false, false, false};
    uint64_t emitted = 0, deposits = 0;
    bool runs = FILM_DEPOSIT_RUNS;                  // the deposit's form (vk_debug_film_deposit_form)
    std::unique_ptr<AdaptState> adapt;              // vk_adapt_enable; null: the film as it always was
};

namespace {

constexpr uint64_t PATHS_MAX = 1ull << 24;
static_assert(VK_PATHS_LIVE == VK_SHADE_SCATTERED && VK_PATHS_CULLED == PATHS_STATUSES - 1, "the statuses the compaction counts");

inline uint32_t paths_wgs(uint64_t n) { return (uint32_t)((n + PATHS_T - 1) / PATHS_T); }

// the words vk_roulette_set and the compaction's second hook refuse a rule with (nullptr: the rule is fine)
const char *roulette_refusal(const vk_roulette_params &rp) {
    if (rp.first_depth < 2u) return "roulette first_depth must be >= 2";
    if (rp.flags != 0u) return "roulette flags must be 0";
    if (!std::isfinite(rp.q_min) || !std::isfinite(rp.q_max)) return "roulette q_min and q_max must be finite";
    if (!(rp.q_min >= 5.9604644775390625e-8f && rp.q_min <= rp.q_max && rp.q_max <= 1.0f)) return "roulette needs 2^-24 <= q_min <= q_max <= 1";
    return nullptr;
}

// the compaction's three launches for A.n > 0 items (A.n_wg set here).  With a rule the first is roulette_count_kernel, which ends or
// rescales the scattered records before it counts them; with a film the third is regen_move_kernel, which deposits what retires into the
// film's sums instead of storing it under its id.
int enqueue_compact(CompactArgs A, hipStream_t st, const vk_film *film = nullptr, const vk_roulette_params *rule = nullptr) {
    A.n_wg = paths_wgs(A.n);
    if (!rule) hipLaunchKernelGGL(paths_count_kernel, dim3(A.n_wg), dim3(PATHS_T), 0, st, A);
    else hipLaunchKernelGGL(roulette_count_kernel, dim3(A.n_wg), dim3(PATHS_T), 0, st, A, RouletteRule{rule->first_depth, rule->q_min, rule->q_max});
    hipLaunchKernelGGL(paths_scan_kernel, dim3(1), dim3(PATHS_SCAN_T), 0, st, A);
    if (!film) {
        hipLaunchKernelGGL(paths_move_kernel, dim3(A.n_wg), dim3(PATHS_T), 0, st, A);
    } else {
        RegenMoveArgs M;
        memset(&M, 0, sizeof(M));
        M.items = A.items; M.ids = A.ids; M.n = A.n; M.rays = A.rays; M.states = A.states; M.ids_out = A.ids_out; M.wg_offsets = A.wg_offsets;
        M.sums = film->sums; M.counters = film->counters;
        M.n_pixels = film->params.width * film->params.height;
        M.accum_clamp = accum_clamp_for(film->params.samples_per_pixel);
        hipLaunchKernelGGL(regen_move_kernel, dim3(A.n_wg), dim3(PATHS_T), 0, st, M);
    }
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

// one launch of trace_paths_kernel for items [0, n)
int enqueue_trace_paths(vk_scene *q, const void *d_rays, void *d_states, void *d_hits, uint64_t n, hipStream_t st) {
    TracePathsArgs A;
    memset(&A, 0, sizeof(A));
    int rc = query_view(q, "a path batch", &A.S);
    if (rc != VK_OK) return rc;
    A.P = q->rays.prov;
    A.rays = static_cast<const float4 *>(d_rays); A.states = static_cast<uint4 *>(d_states); A.hits = static_cast<uint4 *>(d_hits);
    A.n = n;
    const dim3 grid((uint32_t)((n + AOV_BLOCK - 1) / AOV_BLOCK));
    with_walk_variant(q->host->features, [&](auto f) {
        hipLaunchKernelGGL(trace_paths_kernel<decltype(f)::value>, grid, dim3(AOV_BLOCK), 0, st, A);
    });
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

// a compaction's arguments from its device buffers (n_wg is enqueue_compact's)
CompactArgs compact_args(const void *items, const uint32_t *ids, uint64_t n, uint64_t n_ids, void *rays, void *states, uint32_t *ids_out,
                         void *result_state, uint32_t *result_status, uint32_t *wg_counts, uint32_t *wg_offsets, unsigned long long *counts) {
    return CompactArgs{static_cast<const uint4 *>(items), ids, n, n_ids, static_cast<uint4 *>(rays), static_cast<uint4 *>(states), ids_out,
                       static_cast<uint4 *>(result_state), result_status, wg_counts, wg_offsets, counts, 0u};
}
// the handle's compaction of shaded[0, live) and ids[cur] into rays, states and ids[cur ^ 1]; then the counts record, read back (which
// waits for everything enqueued): live and retired[] follow it
CompactArgs paths_compact_args(vk_paths *p) {
    return compact_args(p->shaded, p->ids[p->cur], p->live, p->capacity, p->rays, p->states, p->ids[p->cur ^ 1u], p->result_state,
                        p->result_status, p->wg_counts, p->wg_offsets, p->counts);
}
int paths_take_counts(vk_paths *p, unsigned long long c[5]) {
    HIP_TRY(hipMemcpy(c, p->counts, PATHS_STATUSES * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    p->cur ^= 1u;
    p->live = c[VK_SHADE_SCATTERED];
    for (uint32_t s = 0; s < PATHS_STATUSES; s++) if (s != (uint32_t)VK_SHADE_SCATTERED) p->retired[s] += c[s];
    return VK_OK;
}

// a batch as a begin leaves it: `started` paths of which `live` are live, nothing retired, no bounce run, not regenerating.  Called behind
// every check and every launch of a begin that can fail: a refused call leaves the batch as it was.
void paths_reset(vk_paths *p, const vk_shade_params &sp, uint64_t started, uint64_t live) {
    p->sp = sp; p->begun = true; p->deposited = false; p->splatted = false; p->bucketed = false; p->layered = false; p->begins++; p->cur = 0u; p->started = started; p->live = live; p->bounces = 0u;
    for (uint64_t &r : p->retired) r = 0u;
    p->regen = false; p->regen_film = nullptr; p->regen_win = vk_film_window{}; p->regen_next = 0u; p->regen_total = 0u;
    p->regen_tiles = false; p->regen_first_sample = 0u; p->regen_n_samples = 0u;
}

// what the bounces of one step call add up to: vk_paths_step and vk_regen_step copy it into their info structs
struct BounceTally {
    uint64_t traced, missed, ended, bad;
    double kernel_ms;
    uint32_t launches, bounces;
};
// one bounce of p's live paths (> 0) on the null stream, behind ev0, which the caller has recorded: trace, shade and the compaction — with
// a film, the one that deposits what retires; with the handle's rule set, the one whose count pass applies it — five launches, then the
// counts record and the time from ev0 to ev1
int paths_bounce(vk_paths *p, vk_scene *q, const vk_film *film, BounceTally &T) {
    const uint64_t n = p->live;
    int rc;
    if ((rc = enqueue_trace_paths(q, p->rays, p->states, p->hits, n, nullptr)) != VK_OK) return rc;
    HIP_TRY(hipEventRecord(p->ev_t, nullptr));
    if ((rc = enqueue_shade(q, &p->sp, p->rays, p->hits, p->states, n, p->shaded, nullptr)) != VK_OK) return rc;
    HIP_TRY(hipEventRecord(p->ev_s, nullptr));
    if ((rc = enqueue_compact(paths_compact_args(p), nullptr, film, p->roulette ? &p->rr : nullptr)) != VK_OK) return rc;
    HIP_TRY(hipEventRecord(p->ev1, nullptr));
    unsigned long long c[5];
    if ((rc = paths_take_counts(p, c)) != VK_OK) return rc;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    T.kernel_ms += (double)ms; T.launches += 5u; T.bounces++; T.traced += n;
    T.missed += c[VK_SHADE_MISS]; T.ended += c[VK_SHADE_ENDED]; T.bad += c[VK_SHADE_BAD_HIT];
    p->bounces++;
    return VK_OK;
}

// the cull of p's live paths (> 0, keep not null): the marking pass writes them as the records the compaction reads, and the same
// compaction runs — with a film, the one that deposits the culled paths
int paths_cull(vk_paths *p, const vk_film *film, const uint8_t *keep, const float *scale) {
    const uint64_t n = p->live;
    HIP_TRY(hipSetDevice(first_part(p->scene)->device));
    // keep and scale ride in the hit records' buffer, which holds nothing between two bounces: 5 of its 64 bytes a path
    uint8_t *d_keep = p->hits;
    float *d_scale = reinterpret_cast<float *>(p->hits.get() + (((size_t)p->capacity + 15u) & ~(size_t)15u));
    HIP_TRY(hipMemcpy(d_keep, keep, (size_t)n, hipMemcpyHostToDevice));
    if (scale) HIP_TRY(hipMemcpy(d_scale, scale, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(paths_cull_mark_kernel, dim3(paths_wgs(n)), dim3(PATHS_T), 0, nullptr, reinterpret_cast<const uint4 *>(p->rays.get()),
                       reinterpret_cast<const uint4 *>(p->states.get()), d_keep, scale ? d_scale : nullptr, n,
                       reinterpret_cast<uint4 *>(p->shaded.get()));
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = enqueue_compact(paths_compact_args(p), nullptr, film)) != VK_OK) return rc;
    unsigned long long c[5];
    return paths_take_counts(p, c);
}

// the hooks vk_debug_paths_last_ms and vk_debug_regen_last_ms: the times between the n + 1 events of p's last bounce
int paths_parts_ms(vk_paths *p, const Event *const *ev, int n, double *ms) {
    HIP_TRY(hipSetDevice(first_part(p->scene)->device));
    HIP_TRY(hipEventSynchronize(p->ev1));
    double got[4];
    for (int k = 0; k < n; k++) {
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, *ev[k], *ev[k + 1]));
        got[k] = (double)t;
    }
    for (int k = 0; k < n; k++) ms[k] = got[k];
    return VK_OK;
}

void paths_free(vk_paths *p) {
    (void)hipSetDevice(first_part(p->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a begin's last launch may still run)
    (void)hipGetLastError();
    delete p;
}

// a device buffer of a path batch, a film or the compaction's hook: the first failure of a chain stays in rc and ends it
template <class T>
void handle_alloc(int &rc, DeviceBuffer<T> &b, size_t bytes) {
    if (rc != VK_OK) return;
    const hipError_t e = b.alloc(bytes);
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    rc = fail(e == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP, std::string("hipMalloc (path batch): ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int vk_paths_create(vk_scene *scene, uint64_t capacity, vk_paths **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (capacity < 1u || capacity > PATHS_MAX) return fail(VK_ERR_BAD_ARG, "capacity must be in 1..2^24");
    return guarded([&]() -> int {
        std::unique_ptr<vk_paths, void (*)(vk_paths *)> p(new vk_paths(), paths_free);
        p->scene = scene; p->capacity = capacity;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        const size_t n = (size_t)capacity, n_wg = paths_wgs(capacity);
        int rc = VK_OK;
        handle_alloc(rc, p->rays, n * sizeof(vk_ray)); handle_alloc(rc, p->states, n * sizeof(vk_path_state));
        handle_alloc(rc, p->hits, n * sizeof(vk_hit)); handle_alloc(rc, p->shaded, n * sizeof(vk_shaded));
        handle_alloc(rc, p->ids[0], n * 4u); handle_alloc(rc, p->ids[1], n * 4u);
        handle_alloc(rc, p->result_state, n * sizeof(vk_path_state)); handle_alloc(rc, p->result_status, n * 4u);
        handle_alloc(rc, p->wg_counts, n_wg * PATHS_STATUSES * 4u); handle_alloc(rc, p->wg_offsets, n_wg * 4u);
        handle_alloc(rc, p->counts, PATHS_STATUSES * sizeof(unsigned long long));
        if (rc != VK_OK) return rc;
        if ((rc = p->ev0.create()) != VK_OK || (rc = p->ev1.create()) != VK_OK || (rc = p->ev_t.create()) != VK_OK ||
            (rc = p->ev_s.create()) != VK_OK || (rc = p->ev_e.create()) != VK_OK) return rc;
        *out = p.release();
        return VK_OK;
    });
}

int vk_paths_begin(vk_paths *p, const vk_shade_params *params, const vk_ray *rays, const vk_path_state *states, uint64_t n) {
    return guarded([&]() -> int {
        if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
        const void *in = rays && states ? static_cast<const void *>(rays) : nullptr;
        int rc = check_batch_args(p->scene, params, params ? params->flags : 0u, n, in, p, {"shade", "states"});
        if (rc != VK_OK) return rc;
        if (n > p->capacity) return fail(VK_ERR_BAD_ARG, "n exceeds the path batch's capacity");
        const vk_radiance_params rp = shade_as_radiance(params);
        if ((rc = check_radiance_args(p->scene, &rp, in, n, p)) != VK_OK) return rc;
        if ((rc = check_integrator_for_scene(*p->scene->host, params->integrator)) != VK_OK) return rc;
        vk_scene *q = first_part(p->scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        if (n != 0u) {
            HIP_TRY(hipMemcpy(p->rays, rays, (size_t)n * sizeof(vk_ray), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(p->states, states, (size_t)n * sizeof(vk_path_state), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(paths_iota_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, nullptr, p->ids[0].get(), (uint32_t)n);
            HIP_TRY(hipGetLastError());
        }
        paths_reset(p, *params, n, n);
        return VK_OK;
    });
}

int vk_paths_step(vk_paths *p, uint32_t max_bounces, vk_paths_step_info *info) {
    return guarded([&]() -> int {
        if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
        if (max_bounces == 0u) return fail(VK_ERR_BAD_ARG, "max_bounces must be >= 1");
        if (!p->begun) return fail(VK_ERR_BAD_ARG, "vk_paths_step before vk_paths_begin");
        if (p->regen) return fail(VK_ERR_BAD_ARG, "vk_paths_step on a regenerating path batch (vk_regen_step runs it)");
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(p->scene);
        HIP_TRY(hipSetDevice(q->device));
        BounceTally T{};
        while (p->live != 0u && T.bounces < max_bounces) {
            HIP_TRY(hipEventRecord(p->ev0, nullptr));
            int rc = paths_bounce(p, q, nullptr, T);
            if (rc != VK_OK) return rc;
        }
        vk_paths_step_info I;
        memset(&I, 0, sizeof(I));
        I.traced = T.traced; I.missed = T.missed; I.ended = T.ended; I.bad = T.bad;
        I.bounces = T.bounces; I.kernel_launches = T.launches; I.kernel_ms = T.kernel_ms;
        I.live = p->live;
        I.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = I;
        return VK_OK;
    });
}

int vk_paths_read(vk_paths *p, uint32_t *ids, vk_ray *rays, vk_path_state *states) {
    return guarded([&]() -> int {
        if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
        if (!p->begun) return fail(VK_ERR_BAD_ARG, "vk_paths_read before vk_paths_begin");
        HIP_TRY(hipSetDevice(first_part(p->scene)->device));
        const size_t n = (size_t)p->live;
        if (n == 0u) return VK_OK;
        if (ids) HIP_TRY(hipMemcpy(ids, p->ids[p->cur], n * 4u, hipMemcpyDeviceToHost));
        if (rays) HIP_TRY(hipMemcpy(rays, p->rays, n * sizeof(vk_ray), hipMemcpyDeviceToHost));
        if (states) HIP_TRY(hipMemcpy(states, p->states, n * sizeof(vk_path_state), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_paths_cull(vk_paths *p, const uint8_t *keep, const float *scale) {
    return guarded([&]() -> int {
        if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
        if (!p->begun) return fail(VK_ERR_BAD_ARG, "vk_paths_cull before vk_paths_begin");
        if (p->regen) return fail(VK_ERR_BAD_ARG, "vk_paths_cull on a regenerating path batch (vk_regen_cull culls it)");
        if (p->live == 0u) return VK_OK;
        if (!keep) return fail(VK_ERR_BAD_ARG, "null keep with live paths");
        return paths_cull(p, nullptr, keep, scale);
    });
}

int vk_paths_results(vk_paths *p, vk_path_state *states, uint32_t *status) {
    return guarded([&]() -> int {
        if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
        if (p->regen) return fail(VK_ERR_BAD_ARG, "vk_paths_results on a regenerating path batch (its paths are deposited as they retire)");
        const size_t n = (size_t)p->started, live = (size_t)p->live;
        if (n == 0u || (!states && !status)) return VK_OK;
        HIP_TRY(hipSetDevice(first_part(p->scene)->device));
        if (states) HIP_TRY(hipMemcpy(states, p->result_state, n * sizeof(vk_path_state), hipMemcpyDeviceToHost));
        if (status) HIP_TRY(hipMemcpy(status, p->result_status, n * 4u, hipMemcpyDeviceToHost));
        if (live == 0u) return VK_OK;
        // the live paths: their current states, under their ids
        std::vector<uint32_t> ids(live);
        HIP_TRY(hipMemcpy(ids.data(), p->ids[p->cur], live * 4u, hipMemcpyDeviceToHost));
        std::vector<vk_path_state> cur;
        if (states) {
            cur.resize(live);
            HIP_TRY(hipMemcpy(cur.data(), p->states, live * sizeof(vk_path_state), hipMemcpyDeviceToHost));
        }
        for (size_t j = 0; j < live; j++) {
            if (ids[j] >= n) return fail(VK_ERR_BAD_ARG, "internal error: a live id outside the batch");
            if (states) states[ids[j]] = cur[j];
            if (status) status[ids[j]] = (uint32_t)VK_PATHS_LIVE;
        }
        return VK_OK;
    });
}

int vk_paths_get_info(vk_paths *p, vk_paths_info *out) {
    if (!p || !out) return fail(VK_ERR_BAD_ARG, "null argument (path batch or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(p->scene)->device));
        HIP_TRY(hipStreamSynchronize(nullptr));
        memset(out, 0, sizeof(*out));
        out->capacity = p->capacity; out->started = p->started; out->live = p->live; out->bounces = p->bounces;
        for (int s = 0; s < 5; s++) out->retired[s] = p->retired[s];
        return VK_OK;
    });
}

// the handle's termination rule: host state only, read by the next bounce's compaction
int vk_roulette_set(vk_paths *p, const vk_roulette_params *rp) {
    if (!p) return fail(VK_ERR_BAD_ARG, "null path batch");
    if (!rp) { p->roulette = false; p->rr = vk_roulette_params{}; return VK_OK; }
    if (const char *why = roulette_refusal(*rp)) return fail(VK_ERR_BAD_ARG, why);
    p->rr = *rp; p->roulette = true;
    return VK_OK;
}

int vk_roulette_get(vk_paths *p, vk_roulette_params *out, int *enabled) {
    if (!p || !out || !enabled) return fail(VK_ERR_BAD_ARG, "null argument (path batch, out or enabled)");
    *out = p->rr; *enabled = p->roulette ? 1 : 0;
    return VK_OK;
}

void vk_paths_destroy(vk_paths *p) {
    if (p) paths_free(p);
}

// test hook (vecchio_amd_debug.h): the last bounce's three parts, from the events vk_paths_step records between them
int vk_debug_paths_last_ms(vk_paths *p, double ms[3]) {
    if (!p || !ms) return fail(VK_ERR_BAD_ARG, "null argument (path batch or ms)");
    return guarded([&]() -> int {
        if (p->bounces == 0u) return fail(VK_ERR_BAD_ARG, "no bounce has run since vk_paths_begin");
        const Event *ev[4] = {&p->ev0, &p->ev_t, &p->ev_s, &p->ev1};
        return paths_parts_ms(p, ev, 3, ms);
    });
}

// the two compaction hooks: the production compaction — with a rule, the one whose count pass applies it — on host arrays staged once
static int debug_compact(vk_scene *scene, const vk_roulette_params *rule, const vk_shaded *items, const uint32_t *ids, uint64_t n,
    uint64_t n_ids, vk_ray *rays, vk_path_state *states, uint32_t *ids_out, vk_path_state *result_state, uint32_t *result_status,
    uint64_t counts[5]) {
    return guarded([&]() -> int {
        if (!scene || !counts) return fail(VK_ERR_BAD_ARG, "null argument (scene or counts)");
        if (rule) if (const char *why = roulette_refusal(*rule)) return fail(VK_ERR_BAD_ARG, why);
        if (n > PATHS_MAX || n_ids > (1ull << 26)) return fail(VK_ERR_BAD_ARG, "n exceeds 2^24 or n_ids 2^26");
        if (n != 0u && (!items || !ids || !rays || !states || !ids_out || !result_state || !result_status))
            return fail(VK_ERR_BAD_ARG, "null array with n > 0");
        for (uint64_t i = 0; i < n; i++) if (ids[i] >= n_ids) return fail(VK_ERR_BAD_ARG, "an id is not below n_ids");
        for (int s = 0; s < 5; s++) counts[s] = 0u;
        if (n == 0u) return VK_OK;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        const size_t m = (size_t)n, k = (size_t)n_ids, n_wg = paths_wgs(n);
        DeviceBuffer<uint8_t> d_items, d_rays, d_states, d_rstate;
        DeviceBuffer<uint32_t> d_ids, d_ids_out, d_rstatus, d_wc, d_wo;
        DeviceBuffer<unsigned long long> d_counts;
        int rc = VK_OK;
        handle_alloc(rc, d_items, m * sizeof(vk_shaded)); handle_alloc(rc, d_ids, m * 4u);
        handle_alloc(rc, d_rays, m * sizeof(vk_ray)); handle_alloc(rc, d_states, m * sizeof(vk_path_state));
        handle_alloc(rc, d_ids_out, m * 4u); handle_alloc(rc, d_rstate, k * sizeof(vk_path_state));
        handle_alloc(rc, d_rstatus, k * 4u); handle_alloc(rc, d_wc, n_wg * PATHS_STATUSES * 4u);
        handle_alloc(rc, d_wo, n_wg * 4u); handle_alloc(rc, d_counts, PATHS_STATUSES * sizeof(unsigned long long));
        if (rc != VK_OK) return rc;
        HIP_TRY(hipMemcpy(d_items, items, m * sizeof(vk_shaded), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_ids, ids, m * 4u, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rays, rays, m * sizeof(vk_ray), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_states, states, m * sizeof(vk_path_state), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_ids_out, ids_out, m * 4u, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rstate, result_state, k * sizeof(vk_path_state), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rstatus, result_status, k * 4u, hipMemcpyHostToDevice));
        const CompactArgs A = compact_args(d_items, d_ids, n, n_ids, d_rays, d_states, d_ids_out, d_rstate, d_rstatus, d_wc, d_wo, d_counts);
        if ((rc = enqueue_compact(A, nullptr, nullptr, rule)) != VK_OK) return rc;
        unsigned long long c[5];
        HIP_TRY(hipMemcpy(c, d_counts, sizeof(c), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rays, d_rays, m * sizeof(vk_ray), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(states, d_states, m * sizeof(vk_path_state), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ids_out, d_ids_out, m * 4u, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(result_state, d_rstate, k * sizeof(vk_path_state), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(result_status, d_rstatus, k * 4u, hipMemcpyDeviceToHost));
        for (int s = 0; s < 5; s++) counts[s] = c[s];
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h)
int vk_debug_compact_paths(vk_scene *scene, const vk_shaded *items, const uint32_t *ids, uint64_t n, uint64_t n_ids, vk_ray *rays,
    vk_path_state *states, uint32_t *ids_out, vk_path_state *result_state, uint32_t *result_status, uint64_t counts[5]) {
    return debug_compact(scene, nullptr, items, ids, n, n_ids, rays, states, ids_out, result_state, result_status, counts);
}

// test hook (vecchio_amd_debug.h): its twin with the termination rule in the count pass
int vk_debug_compact_roulette(vk_scene *scene, const vk_roulette_params *rp, const vk_shaded *items, const uint32_t *ids, uint64_t n,
    uint64_t n_ids, vk_ray *rays, vk_path_state *states, uint32_t *ids_out, vk_path_state *result_state, uint32_t *result_status,
    uint64_t counts[5]) {
    if (!rp) return fail(VK_ERR_BAD_ARG, "null argument (roulette parameters)");
    return debug_compact(scene, rp, items, ids, n, n_ids, rays, states, ids_out, result_state, result_status, counts);
}

}  // extern "C"

// ---- films (vk_film_*): a frame's fixed-point sums on the scene's device (devices[0] of a multi-device scene) with its camera and render
// parameters.  film_emit_kernel fills a path batch with camera paths, film_deposit_kernel adds a finished batch to the sums, resolve_kernel
// (vk_render's own, on the whole-image partition) divides; all on the null stream, on buffers and events the handle owns.  Of the batch
// an emit writes what vk_paths_begin writes; a deposit reads its results and sets its `deposited` flag.

namespace {

constexpr uint64_t FILM_MAX_PIXELS = 1ull << 26;

void film_free(vk_film *f) {
    (void)hipSetDevice(first_part(f->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a deposit may still run)
    (void)hipGetLastError();
    delete f;
}

int adapt_zero(vk_film *f);        // (vk_adapt_*, below)

int film_zero(vk_film *f) {
    HIP_TRY(hipMemsetAsync(f->sums, 0, (size_t)f->params.width * f->params.height * 3u * sizeof(unsigned long long), nullptr));
    HIP_TRY(hipMemsetAsync(f->counters, 0, 4u * sizeof(unsigned long long), nullptr));
    f->emitted = 0u; f->deposits = 0u;
    return f->adapt ? adapt_zero(f) : VK_OK;
}

// what vk_film_emit and vk_regen_begin check of their three arguments, in the same words; *n = the window's paths
int film_check_window(const vk_film *film, const vk_paths *batch, const vk_film_window *win, uint64_t *n) {
    if (!film || !batch || !win) return fail(VK_ERR_BAD_ARG, "null argument (film, path batch or window)");
    if (batch->scene != film->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the film");
    const vk_render_params &P = film->params;
    if (win->width == 0u || win->height == 0u || win->n_samples == 0u) return fail(VK_ERR_BAD_ARG, "empty window");
    if ((uint64_t)win->x0 + win->width > P.width || (uint64_t)win->y0 + win->height > P.height)
        return fail(VK_ERR_BAD_ARG, "the window lies outside the film's frame");
    if ((uint64_t)win->first_sample + win->n_samples > P.samples_per_pixel)
        return fail(VK_ERR_BAD_ARG, "first_sample + n_samples exceeds the film's samples_per_pixel");
    // (width * height <= 2^26 and n_samples <= 2^26: the product fits 64 bits)
    *n = (uint64_t)win->width * win->height * win->n_samples;
    return VK_OK;
}

// the film's camera, frame and seed as the emitting kernels take them
RenderConsts film_consts(const vk_film *film) {
    const vk_render_params &P = film->params;
    RenderConsts C;
    memset(&C, 0, sizeof(C));
    C.cam = film->cam;
    C.width = P.width; C.height = P.height; C.spp = P.samples_per_pixel; C.max_depth = P.max_depth;
    C.seed = P.seed; C.integrator = P.integrator; C.background = P.background;
    C.bg[0] = P.background_color[0]; C.bg[1] = P.background_color[1]; C.bg[2] = P.background_color[2];
    return C;
}

// a window as the emitting kernels take it
EmitWindow emit_window(const vk_film_window &w) { return EmitWindow{w.x0, w.y0, w.width, w.first_sample, w.n_samples}; }

// the film's shade parameters: what a batch it fills is shaded with
vk_shade_params film_shade_params(const vk_film *film) {
    const vk_render_params &P = film->params;
    vk_shade_params sp;
    memset(&sp, 0, sizeof(sp));
    sp.max_depth = P.max_depth; sp.integrator = P.integrator; sp.background = P.background;
    sp.background_color[0] = P.background_color[0]; sp.background_color[1] = P.background_color[1]; sp.background_color[2] = P.background_color[2];
    return sp;
}

}  // namespace

extern "C" {

int vk_film_create(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, vk_film **out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    int rc = check_render_args(scene, cam, params);
    if (rc != VK_OK) return rc;
    if ((params->tile_world ? params->tile_world : 1u) > 1u) return fail(VK_ERR_BAD_ARG, "a film holds the whole image (tile_world must be 0 or 1)");
    if (params->output_format != VK_OUTPUT_F32) return fail(VK_ERR_BAD_ARG, "a film is f32 only (output_format must be VK_OUTPUT_F32)");
    if (params->max_depth == 0u) return fail(VK_ERR_BAD_ARG, "max_depth must be >= 1 (vk_shade_hits' contract starts no path at max_depth 0)");
    if ((uint64_t)params->width * params->height > FILM_MAX_PIXELS) return fail(VK_ERR_BAD_ARG, "width * height exceeds 2^26");
    return guarded([&]() -> int {
        std::unique_ptr<vk_film, void (*)(vk_film *)> f(new vk_film(), film_free);
        f->scene = scene; f->cam = *cam; f->params = *params;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, f->sums, (size_t)params->width * params->height * 3u * sizeof(unsigned long long));
        handle_alloc(r, f->counters, 4u * sizeof(unsigned long long));
        if (r != VK_OK) return r;
        for (Event &e : f->ev) if ((r = e.create()) != VK_OK) return r;
        if ((r = film_zero(f.get())) != VK_OK) return r;
        *out = f.release();
        return VK_OK;
    });
}

int vk_film_emit(vk_film *film, vk_paths *batch, const vk_film_window *win) {
    return guarded([&]() -> int {
        uint64_t n = 0;
        int rc = film_check_window(film, batch, win, &n);
        if (rc != VK_OK) return rc;
        if (n > batch->capacity) return fail(VK_ERR_BAD_ARG, "the window's paths exceed the path batch's capacity");
        vk_scene *q = first_part(film->scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        FilmEmitArgs A;
        memset(&A, 0, sizeof(A));
        A.C = film_consts(film);
        A.rays = reinterpret_cast<uint4 *>(batch->rays.get()); A.states = reinterpret_cast<uint4 *>(batch->states.get());
        A.ids = batch->ids[0];
        A.W = emit_window(*win);
        A.n = (uint32_t)n;                           // (capacity <= 2^24)
        HIP_TRY(hipEventRecord(film->ev[0], nullptr));
        hipLaunchKernelGGL(film_emit_kernel, dim3((uint32_t)((n + FILM_T - 1) / FILM_T)), dim3(FILM_T), 0, nullptr, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(film->ev[1], nullptr));
        film->timed[0] = true;
        film->emitted += n;
        paths_reset(batch, film_shade_params(film), n, n);
        return VK_OK;
    });
}

int vk_film_deposit(vk_film *film, vk_paths *batch) {
    return guarded([&]() -> int {
        if (!film || !batch) return fail(VK_ERR_BAD_ARG, "null argument (film or path batch)");
        if (batch->scene != film->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the film");
        if (!batch->begun) return fail(VK_ERR_BAD_ARG, "vk_film_deposit before vk_paths_begin or vk_film_emit");
        if (batch->regen) return fail(VK_ERR_BAD_ARG, "vk_film_deposit on a regenerating path batch (its paths are deposited as they retire)");
        if (batch->live != 0u) return fail(VK_ERR_BAD_ARG, "the path batch has live paths (step or cull them first)");
        if (batch->deposited) return fail(VK_ERR_BAD_ARG, "the path batch has been deposited since its last begin or emit");
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const uint64_t n = batch->started;
        HIP_TRY(hipEventRecord(film->ev[2], nullptr));
        if (n != 0u) {
            FilmDepositArgs A;
            memset(&A, 0, sizeof(A));
            A.result_state = reinterpret_cast<const uint4 *>(batch->result_state.get()); A.result_status = batch->result_status;
            A.sums = film->sums; A.counters = film->counters;
            A.n = (uint32_t)n; A.n_pixels = film->params.width * film->params.height;
            A.accum_clamp = accum_clamp_for(film->params.samples_per_pixel);
            const dim3 grid((uint32_t)((n + FILM_T - 1) / FILM_T));
            if (film->runs) hipLaunchKernelGGL(film_deposit_kernel<true>, grid, dim3(FILM_T), 0, nullptr, A);
            else hipLaunchKernelGGL(film_deposit_kernel<false>, grid, dim3(FILM_T), 0, nullptr, A);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(film->ev[3], nullptr));
        film->timed[1] = true;
        film->deposits++;
        batch->deposited = true;
        return VK_OK;
    });
}

int vk_film_resolve(vk_film *film, uint32_t n, float *rgb_out) {
    return guarded([&]() -> int {
        if (!film || !rgb_out) return fail(VK_ERR_BAD_ARG, "null argument (film or rgb_out)");
        if (n == 0u) return fail(VK_ERR_BAD_ARG, "n must be >= 1");
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const vk_render_params &P = film->params;
        const size_t bytes = (size_t)P.width * P.height * 3u * sizeof(float);
        if (!film->out) {
            int rc = VK_OK;
            handle_alloc(rc, film->out, bytes);
            if (rc != VK_OK) return rc;
        }
        const uint32_t n_pixels = P.width * P.height;
        HIP_TRY(hipEventRecord(film->ev[4], nullptr));
        hipLaunchKernelGGL(resolve_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, nullptr,
                           reinterpret_cast<const long long *>(film->sums.get()), film->out.get(), P.width, P.height, n, (P.width + TILE - 1) / TILE, 0u, 1u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(film->ev[5], nullptr));
        film->timed[2] = true;
        HIP_TRY(hipMemcpy(rgb_out, film->out, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_film_reset(vk_film *film, const vk_camera *cam) {
    if (!film) return fail(VK_ERR_BAD_ARG, "null film");
    if (cam) {
        int rc = check_render_args(film->scene, cam, &film->params);
        if (rc != VK_OK) return rc;
    }
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        int rc = film_zero(film);
        if (rc != VK_OK) return rc;
        if (cam) film->cam = *cam;
        return VK_OK;
    });
}

int vk_film_get_info(vk_film *film, vk_film_info *out) {
    if (!film || !out) return fail(VK_ERR_BAD_ARG, "null argument (film or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        unsigned long long c[4];
        HIP_TRY(hipMemcpy(c, film->counters, sizeof(c), hipMemcpyDeviceToHost));      // (waits for the null stream)
        memset(out, 0, sizeof(*out));
        out->width = film->params.width; out->height = film->params.height; out->samples_per_pixel = film->params.samples_per_pixel;
        out->emitted = film->emitted; out->deposited = c[0]; out->dropped = c[1]; out->clamped = c[2]; out->skipped = c[3];
        out->deposits = film->deposits;
        return VK_OK;
    });
}

void vk_film_destroy(vk_film *film) {
    if (film) film_free(film);
}

// test hook (vecchio_amd_debug.h): the raw sums
int vk_debug_film_sums(vk_film *film, long long *sums) {
    if (!film || !sums) return fail(VK_ERR_BAD_ARG, "null argument (film or sums)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        HIP_TRY(hipMemcpy(sums, film->sums, (size_t)film->params.width * film->params.height * 3u * sizeof(long long), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the last emit, deposit and resolve, from the events recorded around each; 0 for one not yet run
int vk_debug_film_last_ms(vk_film *film, double ms[3]) {
    if (!film || !ms) return fail(VK_ERR_BAD_ARG, "null argument (film or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        double got[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; k++) {
            if (!film->timed[k]) continue;
            HIP_TRY(hipEventSynchronize(film->ev[2 * k + 1]));
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, film->ev[2 * k], film->ev[2 * k + 1]));
            got[k] = (double)t;
        }
        for (int k = 0; k < 3; k++) ms[k] = got[k];
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the deposit's form from the next vk_film_deposit on
int vk_debug_film_deposit_form(vk_film *film, int form) {
    if (!film) return fail(VK_ERR_BAD_ARG, "null film");
    if (form != VK_DEBUG_FILM_DEPOSIT_PLAIN && form != VK_DEBUG_FILM_DEPOSIT_RUNS) return fail(VK_ERR_BAD_ARG, "unknown deposit form");
    film->runs = form == VK_DEBUG_FILM_DEPOSIT_RUNS;
    return VK_OK;
}

}  // extern "C"

// ---- regeneration (vk_regen_*): a path batch refilled from a film's window as its paths retire.  A bounce is at most six launches on the
// null stream — regen_emit_kernel (the top-up), trace_paths_kernel, shade_hits_kernel, paths_count_kernel, paths_scan_kernel and
// regen_move_kernel, which deposits the retired paths into the film and compacts the survivors (a tile run, vk_adapt_begin below, tops up
// with adapt_emit_kernel instead) — and one readback of the counts record,
// from which the host computes the next top-up.  The state of a run lives in vk_paths' host-side regen fields; a batch's device memory is
// what it was.
namespace {

constexpr uint64_t REGEN_MAX = 1ull << 32;         // ids are 32 bits

// vk_regen_step's and vk_regen_cull's argument checks
int regen_check(const vk_film *film, const vk_paths *batch, const char *who) {
    if (!film || !batch) return fail(VK_ERR_BAD_ARG, "null argument (film or path batch)");
    if (batch->scene != film->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the film");
    if (!batch->begun || !batch->regen) return fail(VK_ERR_BAD_ARG, std::string(who) + " on a path batch that is not regenerating (vk_regen_begin first)");
    if (batch->regen_film != film) return fail(VK_ERR_BAD_ARG, "the run was begun with another film");
    return VK_OK;
}

// a run whose window is emitted and whose last path has retired: nothing is left to deposit
void regen_note_finished(vk_paths *p) {
    if (p->live == 0u && p->regen_next == p->regen_total) p->deposited = true;
}

// the film's tile set as the kernels of vk_adapt.hip index it
AdaptTiles adapt_tiles(const vk_film *film) {
    const AdaptState &a = *film->adapt;
    const vk_render_params &P = film->params;
    return AdaptTiles{a.list, a.prefix, a.n_active, P.width, P.height, a.tiles_x, (P.width % TILE == 0u && P.height % TILE == 0u) ? 1u : 0u};
}

// the top-up of a tile run (vk_adapt_begin): the run's next m paths behind p's survivors
AdaptEmitArgs adapt_emit_args(const vk_film *film, const vk_paths *p, uint32_t m) {
    AdaptEmitArgs A;
    memset(&A, 0, sizeof(A));
    A.C = film_consts(film);
    A.rays = reinterpret_cast<uint4 *>(p->rays.get()); A.states = reinterpret_cast<uint4 *>(p->states.get());
    A.ids = p->ids[p->cur];                                  // (the last compaction's flip is behind us)
    A.T = adapt_tiles(film);
    A.first_sample = p->regen_first_sample; A.n_samples = p->regen_n_samples;
    A.first = (uint32_t)p->regen_next; A.slot0 = (uint32_t)p->live; A.m = m;      // (total < 2^32, capacity <= 2^24)
    return A;
}

}  // namespace

extern "C" {

int vk_regen_begin(vk_film *film, vk_paths *batch, const vk_film_window *win) {
    return guarded([&]() -> int {
        uint64_t total = 0;
        int rc = film_check_window(film, batch, win, &total);
        if (rc != VK_OK) return rc;
        if (total >= REGEN_MAX) return fail(VK_ERR_BAD_ARG, "the window's paths exceed 2^32 - 1 (split it by sample ranges)");
        vk_scene *q = first_part(film->scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        paths_reset(batch, film_shade_params(film), 0u, 0u);
        batch->regen = true; batch->regen_film = film; batch->regen_win = *win; batch->regen_total = total;
        return VK_OK;
    });
}

int vk_regen_step(vk_film *film, vk_paths *batch, uint32_t max_bounces, vk_regen_info *info) {
    return guarded([&]() -> int {
        int rc = regen_check(film, batch, "vk_regen_step");
        if (rc != VK_OK) return rc;
        if (max_bounces == 0u) return fail(VK_ERR_BAD_ARG, "max_bounces must be >= 1");
        const auto t0 = std::chrono::steady_clock::now();
        vk_paths *p = batch;
        vk_scene *q = first_part(p->scene);
        HIP_TRY(hipSetDevice(q->device));
        BounceTally T{};
        uint64_t emitted = 0;
        while (T.bounces < max_bounces) {
            // 1. top up: the window's next m paths behind the survivors, ids = their numbers (above every live id: live order stays ascending)
            const uint64_t m = std::min(p->capacity - p->live, p->regen_total - p->regen_next);
            if (p->live + m == 0u) break;                                // 2. the run is finished
            HIP_TRY(hipEventRecord(p->ev0, nullptr));
            if (m != 0u) {
                if (p->regen_tiles) {                                    // a tile run (vk_adapt_begin): adapt_emit_kernel
                    launch_adapt_emit(adapt_emit_args(film, p, (uint32_t)m));
                } else {
                    RegenEmitArgs A;
                    memset(&A, 0, sizeof(A));
                    A.C = film_consts(film);
                    A.rays = reinterpret_cast<uint4 *>(p->rays.get()); A.states = reinterpret_cast<uint4 *>(p->states.get());
                    A.ids = p->ids[p->cur];                              // (the last compaction's flip is behind us)
                    A.W = emit_window(p->regen_win);
                    A.first = (uint32_t)p->regen_next; A.slot0 = (uint32_t)p->live; A.m = (uint32_t)m;  // (total < 2^32, capacity <= 2^24)
                    hipLaunchKernelGGL(regen_emit_kernel, dim3((uint32_t)((m + FILM_T - 1) / FILM_T)), dim3(FILM_T), 0, nullptr, A);
                }
                HIP_TRY(hipGetLastError());
                p->live += m; p->regen_next += m; p->started = p->regen_next;
                film->emitted += m; emitted += m;
                T.launches++;
            }
            HIP_TRY(hipEventRecord(p->ev_e, nullptr));
            // 3. trace, shade, retire into the film and compact
            if ((rc = paths_bounce(p, q, film, T)) != VK_OK) return rc;
        }
        regen_note_finished(p);
        vk_regen_info I;
        memset(&I, 0, sizeof(I));
        I.traced = T.traced; I.emitted = emitted; I.missed = T.missed; I.ended = T.ended; I.bad = T.bad;
        I.bounces = T.bounces; I.kernel_launches = T.launches; I.kernel_ms = T.kernel_ms;
        I.live = p->live; I.remaining = p->regen_total - p->regen_next;
        I.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = I;
        return VK_OK;
    });
}

int vk_regen_cull(vk_film *film, vk_paths *batch, const uint8_t *keep, const float *scale) {
    return guarded([&]() -> int {
        int rc = regen_check(film, batch, "vk_regen_cull");
        if (rc != VK_OK) return rc;
        if (batch->live == 0u) return VK_OK;
        if (!keep) return fail(VK_ERR_BAD_ARG, "null keep with live paths");
        if ((rc = paths_cull(batch, film, keep, scale)) != VK_OK) return rc;
        regen_note_finished(batch);
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the last regenerating bounce's four parts, from the events vk_regen_step records between them
int vk_debug_regen_last_ms(vk_paths *p, double ms[4]) {
    if (!p || !ms) return fail(VK_ERR_BAD_ARG, "null argument (path batch or ms)");
    return guarded([&]() -> int {
        if (!p->regen || p->bounces == 0u) return fail(VK_ERR_BAD_ARG, "no bounce has run since vk_regen_begin");
        const Event *ev[5] = {&p->ev0, &p->ev_e, &p->ev_t, &p->ev_s, &p->ev1};
        return paths_parts_ms(p, ev, 4, ms);
    });
}

}  // extern "C"

// ---- a film's error moments and adaptive regeneration (vk_adapt_*): vk_progress' batch-means moments and tile map kept next to a film's
// sums.  The kernels are vk_adapt.hip's (vk_adapt.h): adapt_emit_kernel tops a tile run up in vk_regen_step, adapt_close_kernel folds and
// judges, adapt_count_kernel and adapt_scatter_kernel rebuild the list of active tiles with its pixel prefix, adapt_resolve_kernel and
// adapt_stderr_kernel write the images.  All on the null stream of the film's device; the host keeps samples_done, steps and the counts
// of the one record a rebuild sends back.
namespace {

// the words vk_progress_set_adaptive refuses parameters with (nullptr: they are fine)
const char *adaptive_refusal(const vk_adaptive_params &ap) {
    if (ap.min_steps < 2) return "min_steps must be >= 2 (the error estimate needs two windows)";
    if (!(std::isfinite(ap.abs_tol) && ap.abs_tol >= 0.0f && std::isfinite(ap.rel_tol) && ap.rel_tol >= 0.0f))
        return "abs_tol and rel_tol must be finite and >= 0";
    return nullptr;
}

// the list and its prefix from the tile map as it stands, then the record: n_active and px_active follow it (waits)
int adapt_rebuild(vk_film *f) {
    AdaptState &a = *f->adapt;
    AdaptListArgs L;
    memset(&L, 0, sizeof(L));
    L.tile_n = a.tile_n; L.list = a.list; L.prefix = a.prefix; L.block_tiles = a.block_tiles; L.block_px = a.block_px; L.record = a.record;
    L.tiles = a.tiles; L.width = f->params.width; L.height = f->params.height; L.tiles_x = a.tiles_x;
    launch_adapt_list(L);
    HIP_TRY(hipGetLastError());
    unsigned long long rec[2];
    HIP_TRY(hipMemcpy(rec, a.record, sizeof(rec), hipMemcpyDeviceToHost));
    a.n_active = (uint32_t)rec[0]; a.px_active = rec[1];
    return VK_OK;
}

// back to sample 0 with every tile active (vk_film_reset; the film's device is current)
int adapt_zero(vk_film *f) {
    AdaptState &a = *f->adapt;
    const size_t words = (size_t)f->params.width * f->params.height * 3u;
    HIP_TRY(hipMemsetAsync(a.prev, 0, words * sizeof(long long), nullptr));
    HIP_TRY(hipMemsetAsync(a.m2, 0, words * sizeof(double), nullptr));
    HIP_TRY(hipMemsetAsync(a.tile_n, 0, (size_t)a.tiles * sizeof(uint32_t), nullptr));
    HIP_TRY(hipMemsetAsync(a.tile_k, 0, (size_t)a.tiles * sizeof(uint32_t), nullptr));
    a.done = 0u; a.steps = 0u; a.samples_rendered = 0u;
    return adapt_rebuild(f);
}

int adapt_check(const vk_film *film, const char *who) {
    if (!film) return fail(VK_ERR_BAD_ARG, "null film");
    if (!film->adapt) return fail(VK_ERR_BAD_ARG, std::string(who) + " on a film without vk_adapt_enable");
    return VK_OK;
}

AdaptImageArgs adapt_image_args(vk_film *film) {
    const AdaptState &a = *film->adapt;
    AdaptImageArgs A;
    memset(&A, 0, sizeof(A));
    A.prev = a.prev; A.m2 = a.m2; A.tile_n = a.tile_n; A.tile_k = a.tile_k; A.out = film->out;
    A.width = film->params.width; A.height = film->params.height; A.tiles_x = a.tiles_x; A.done = a.done; A.steps = a.steps;
    return A;
}

// the film's image buffer on the device (vk_film_resolve's), made on first use
int film_out(vk_film *film, size_t bytes) {
    int rc = VK_OK;
    if (!film->out) handle_alloc(rc, film->out, bytes);
    return rc;
}

}  // namespace

extern "C" {

int vk_adapt_enable(vk_film *film, const vk_adaptive_params *ap) {
    if (!film) return fail(VK_ERR_BAD_ARG, "null film");
    if (ap) if (const char *why = adaptive_refusal(*ap)) return fail(VK_ERR_BAD_ARG, why);
    if (film->emitted != 0u || film->deposits != 0u)
        return fail(VK_ERR_BAD_ARG, "vk_adapt_enable comes before the film's first emit or deposit since create / reset");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        if (!film->adapt) {
            const vk_render_params &P = film->params;
            std::unique_ptr<AdaptState> a(new AdaptState());
            a->tiles_x = (P.width + TILE - 1) / TILE;
            a->tiles = a->tiles_x * ((P.height + TILE - 1) / TILE);
            const size_t words = (size_t)P.width * P.height * 3u, nb = ((size_t)a->tiles + 1023u) / 1024u;
            int rc = VK_OK;
            handle_alloc(rc, a->prev, words * sizeof(long long)); handle_alloc(rc, a->m2, words * sizeof(double));
            handle_alloc(rc, a->tile_n, (size_t)a->tiles * 4u); handle_alloc(rc, a->tile_k, (size_t)a->tiles * 4u);
            handle_alloc(rc, a->list, (size_t)a->tiles * 4u); handle_alloc(rc, a->prefix, ((size_t)a->tiles + 1u) * 4u);
            handle_alloc(rc, a->block_tiles, nb * 4u); handle_alloc(rc, a->block_px, nb * 4u);
            handle_alloc(rc, a->record, 2u * sizeof(unsigned long long));
            if (rc != VK_OK) return rc;                  // (the film as it was: `a` lets go of what it got)
            film->adapt = std::move(a);
            if ((rc = adapt_zero(film)) != VK_OK) { film->adapt.reset(); return rc; }
        }
        film->adapt->judged = ap != nullptr;
        film->adapt->ap = ap ? *ap : vk_adaptive_params{};
        return VK_OK;
    });
}

int vk_adapt_begin(vk_film *film, vk_paths *batch, uint32_t n_samples) {
    return guarded([&]() -> int {
        if (!film || !batch) return fail(VK_ERR_BAD_ARG, "null argument (film or path batch)");
        int rc = adapt_check(film, "vk_adapt_begin");
        if (rc != VK_OK) return rc;
        if (batch->scene != film->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the film");
        const AdaptState &a = *film->adapt;
        if (n_samples == 0u) return fail(VK_ERR_BAD_ARG, "n_samples must be >= 1");
        if ((uint64_t)a.done + n_samples > film->params.samples_per_pixel)
            return fail(VK_ERR_BAD_ARG, "samples_done + n_samples exceeds the film's samples_per_pixel");
        // (pixels <= 2^26 and n_samples <= 2^32: the product fits 64 bits)
        const uint64_t total = a.px_active * n_samples;
        if (total >= REGEN_MAX) return fail(VK_ERR_BAD_ARG, "the tile window's paths exceed 2^32 - 1 (fewer samples a run)");
        vk_scene *q = first_part(film->scene);
        HIP_TRY(hipSetDevice(q->device));
        if ((rc = ensure_provenance(q)) != VK_OK) return rc;
        paths_reset(batch, film_shade_params(film), 0u, 0u);
        batch->regen = true; batch->regen_film = film; batch->regen_total = total;
        batch->regen_tiles = true; batch->regen_first_sample = a.done; batch->regen_n_samples = n_samples;
        regen_note_finished(batch);                        // (no tile active: finished at once)
        return VK_OK;
    });
}

int vk_adapt_close(vk_film *film, uint32_t n_samples, vk_adapt_info *info) {
    return guarded([&]() -> int {
        int rc = adapt_check(film, "vk_adapt_close");
        if (rc != VK_OK) return rc;
        AdaptState &a = *film->adapt;
        if (n_samples == 0u) return fail(VK_ERR_BAD_ARG, "n_samples must be >= 1");
        if ((uint64_t)a.done + n_samples > film->params.samples_per_pixel)
            return fail(VK_ERR_BAD_ARG, "samples_done + n_samples exceeds the film's samples_per_pixel");
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const uint32_t done = a.done + n_samples, steps = a.steps + 1u;
        if (a.n_active != 0u) {
            AdaptCloseArgs A;
            memset(&A, 0, sizeof(A));
            A.sums = reinterpret_cast<const long long *>(film->sums.get()); A.prev = a.prev; A.m2 = a.m2;
            A.list = a.list; A.tile_n = a.tile_n; A.tile_k = a.tile_k;
            A.n_active = a.n_active; A.width = film->params.width; A.height = film->params.height; A.tiles_x = a.tiles_x;
            A.window = n_samples; A.done = done; A.steps = steps;
            A.gate = (a.judged && done >= a.ap.min_samples && steps >= a.ap.min_steps) ? 1u : 0u;
            A.abs_tol = a.ap.abs_tol; A.rel_tol = a.ap.rel_tol;
            launch_adapt_close(A);
            HIP_TRY(hipGetLastError());
            const uint64_t px = a.px_active;
            if (A.gate) { if ((rc = adapt_rebuild(film)) != VK_OK) return rc; }      // (no gate: no tile changed, the list stands)
            a.samples_rendered += px * n_samples;
        }
        a.done = done; a.steps = steps;
        if (info) {
            vk_adapt_info I;
            memset(&I, 0, sizeof(I));
            I.samples_done = a.done; I.steps = a.steps; I.tiles_total = a.tiles; I.tiles_active = a.n_active;
            I.pixels_active = a.px_active; I.samples_rendered = a.samples_rendered;
            *info = I;
        }
        return VK_OK;
    });
}

int vk_adapt_resolve(vk_film *film, float *rgb_out) {
    return guarded([&]() -> int {
        if (!film || !rgb_out) return fail(VK_ERR_BAD_ARG, "null argument (film or rgb_out)");
        int rc = adapt_check(film, "vk_adapt_resolve");
        if (rc != VK_OK) return rc;
        if (film->adapt->done == 0u) return fail(VK_ERR_BAD_ARG, "vk_adapt_resolve before the first vk_adapt_close");
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const size_t bytes = (size_t)film->params.width * film->params.height * 3u * sizeof(float);
        if ((rc = film_out(film, bytes)) != VK_OK) return rc;
        launch_adapt_resolve(adapt_image_args(film));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(rgb_out, film->out, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_adapt_stderr(vk_film *film, float *out) {
    return guarded([&]() -> int {
        if (!film || !out) return fail(VK_ERR_BAD_ARG, "null argument (film or out)");
        int rc = adapt_check(film, "vk_adapt_stderr");
        if (rc != VK_OK) return rc;
        if (film->adapt->steps < 2u) return fail(VK_ERR_BAD_ARG, "the standard error needs two closes or more");
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const size_t bytes = (size_t)film->params.width * film->params.height * 3u * sizeof(float);
        if ((rc = film_out(film, bytes)) != VK_OK) return rc;
        launch_adapt_stderr(adapt_image_args(film));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out, film->out, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_adapt_tile_samples(vk_film *film, uint32_t *out, vk_adaptive_info *info) {
    return guarded([&]() -> int {
        int rc = adapt_check(film, "vk_adapt_tile_samples");
        if (rc != VK_OK) return rc;
        const AdaptState &a = *film->adapt;
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        if (out) {
            HIP_TRY(hipMemcpy(out, a.tile_n, (size_t)a.tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t t = 0; t < a.tiles; t++) if (out[t] == 0u) out[t] = a.done;
        }
        if (info) {
            memset(info, 0, sizeof(*info));
            info->tiles_total = a.tiles; info->tiles_active = a.n_active; info->samples_rendered = a.samples_rendered;
        }
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the sums at the last close and the moments
int vk_debug_adapt_moments(vk_film *film, long long *run, double *m2) {
    return guarded([&]() -> int {
        int rc = adapt_check(film, "vk_debug_adapt_moments");
        if (rc != VK_OK) return rc;
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        const size_t words = (size_t)film->params.width * film->params.height * 3u;
        if (run) HIP_TRY(hipMemcpy(run, film->adapt->prev, words * sizeof(long long), hipMemcpyDeviceToHost));
        if (m2) HIP_TRY(hipMemcpy(m2, film->adapt->m2, words * sizeof(double), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): a tile map imposed, the list rebuilt from it
int vk_debug_adapt_set_tiles(vk_film *film, const uint32_t *tile_n, const uint32_t *tile_k) {
    return guarded([&]() -> int {
        if (!film || !tile_n || !tile_k) return fail(VK_ERR_BAD_ARG, "null argument (film, tile_n or tile_k)");
        int rc = adapt_check(film, "vk_debug_adapt_set_tiles");
        if (rc != VK_OK) return rc;
        AdaptState &a = *film->adapt;
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        HIP_TRY(hipMemcpy(a.tile_n, tile_n, (size_t)a.tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(a.tile_k, tile_k, (size_t)a.tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
        if ((rc = adapt_rebuild(film)) != VK_OK) return rc;
        const vk_render_params &P = film->params;
        a.samples_rendered = 0u;
        for (uint32_t t = 0; t < a.tiles; t++) {
            const uint32_t tx = (t % a.tiles_x) * TILE, ty = (t / a.tiles_x) * TILE;
            const uint64_t px = (uint64_t)std::min<uint32_t>(TILE, P.width - tx) * std::min<uint32_t>(TILE, P.height - ty);
            a.samples_rendered += px * (tile_n[t] ? tile_n[t] : a.done);
        }
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): adapt_locate on the device for paths first .. first + m of a tile run over the current tile set
int vk_debug_adapt_sequence(vk_film *film, uint32_t n_samples, uint64_t first, uint32_t m, uint32_t *pixel_out, uint32_t *sample_out) {
    return guarded([&]() -> int {
        if (!film || !pixel_out || !sample_out) return fail(VK_ERR_BAD_ARG, "null argument (film, pixel_out or sample_out)");
        int rc = adapt_check(film, "vk_debug_adapt_sequence");
        if (rc != VK_OK) return rc;
        const AdaptState &a = *film->adapt;
        if (n_samples == 0u) return fail(VK_ERR_BAD_ARG, "n_samples must be >= 1");
        const uint64_t total = a.px_active * n_samples;
        if (total >= REGEN_MAX || (uint64_t)m > PATHS_MAX || first > total || (uint64_t)m > total - first)
            return fail(VK_ERR_BAD_ARG, "first + m lies beyond the tile run's paths (or m > 2^24, or the run has 2^32 paths or more)");
        if (m == 0u) return VK_OK;
        HIP_TRY(hipSetDevice(first_part(film->scene)->device));
        DeviceBuffer<uint32_t> d;
        handle_alloc(rc, d, (size_t)m * 2u * sizeof(uint32_t));
        if (rc != VK_OK) return rc;
        AdaptSequenceArgs A;
        memset(&A, 0, sizeof(A));
        A.T = adapt_tiles(film);
        A.first_sample = a.done; A.n_samples = n_samples; A.first = (uint32_t)first; A.m = m;
        A.pixel_out = d.get(); A.sample_out = d.get() + m;
        launch_adapt_sequence(A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(pixel_out, A.pixel_out, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sample_out, A.sample_out, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

}  // extern "C"

// ---- reconstruction filters (vk_splat_*): a frame's filtered fixed-point sums — r, g, b and the weight per pixel — on the scene's device
// (devices[0] of a multi-device scene).  splat_deposit_kernel adds a finished batch, splat_resolve_kernel divides (vk_splat.hip); all on
// the null stream, on buffers and events the handle owns.  Of the batch a deposit reads its results and sets its `splatted` flag; nothing
// of the scene handle is read but its device.
struct vk_splat {
    vk_scene *scene = nullptr;                      // as handed to vk_splat_create
    uint32_t width = 0, height = 0, spp = 0;
    vk_splat_params sp{};
    SplatFilter filter{};
    float accum_clamp = 0.0f;
    DeviceBuffer<unsigned long long> sums;          // [width * height * 4], two's complement
    DeviceBuffer<unsigned long long> counters;      // deposited, dropped, clamped, skipped, contributions, in SPLAT_STRIPES stripes
    DeviceBuffer<float> out;                        // the resolved frame on its way to the host (allocated by the first resolve)
    DeviceBuffer<float> positions;                  // the caller's positions on their way to the device (grown by a deposit that has some)
    size_t positions_cap = 0;                       // floats
    Event ev[4];                                    // around the last deposit and resolve
    bool timed[2] = {false, false};
    uint64_t deposits = 0;
    bool tiled = SPLAT_DEFAULT_TILED;               // the deposit's form (vk_debug_splat_form)
};

namespace {

constexpr size_t SPLAT_COUNTER_BYTES = (size_t)SPLAT_STRIPES * SPLAT_STRIPE_WORDS * sizeof(unsigned long long);

void splat_free(vk_splat *s) {
    (void)hipSetDevice(first_part(s->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a deposit may still run)
    (void)hipGetLastError();
    delete s;
}

int splat_zero(vk_splat *s) {
    HIP_TRY(hipMemsetAsync(s->sums, 0, (size_t)s->width * s->height * 4u * sizeof(unsigned long long), nullptr));
    HIP_TRY(hipMemsetAsync(s->counters, 0, SPLAT_COUNTER_BYTES, nullptr));
    s->deposits = 0u;
    return VK_OK;
}

const char *splat_refusal(const vk_splat_params &sp) {
    if (sp.filter != VK_SPLAT_BOX && sp.filter != VK_SPLAT_TENT && sp.filter != VK_SPLAT_MITCHELL) return "unknown filter";
    if (!std::isfinite(sp.radius) || !(sp.radius >= 0.5f && sp.radius <= 2.0f)) return "radius must be finite and in [0.5, 2]";
    if (sp.filter == VK_SPLAT_MITCHELL)
        for (float v : {sp.b, sp.c})
            if (!std::isfinite(v) || !(v >= 0.0f && v <= 1.0f)) return "b and c must be finite and in [0, 1]";
    return nullptr;
}

}  // namespace

extern "C" {

int vk_splat_default_params(vk_splat_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    out->filter = VK_SPLAT_MITCHELL; out->radius = 2.0f; out->b = 1.0f / 3.0f; out->c = 1.0f / 3.0f;
    return VK_OK;
}

int vk_splat_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, const vk_splat_params *sp, vk_splat **out) {
    if (!scene || !sp || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene, params or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if ((uint64_t)width * height > FILM_MAX_PIXELS) return fail(VK_ERR_BAD_ARG, "width * height exceeds 2^26");
    if (samples_per_pixel == 0u || samples_per_pixel > (1u << 26)) return fail(VK_ERR_BAD_ARG, "samples_per_pixel must be in 1..2^26");
    if (const char *why = splat_refusal(*sp)) return fail(VK_ERR_BAD_ARG, why);
    return guarded([&]() -> int {
        std::unique_ptr<vk_splat, void (*)(vk_splat *)> s(new vk_splat(), splat_free);
        s->scene = scene; s->width = width; s->height = height; s->spp = samples_per_pixel; s->sp = *sp;
        if (sp->filter != VK_SPLAT_MITCHELL) { s->sp.b = 0.0f; s->sp.c = 0.0f; }
        s->filter = splat_filter_for(sp->filter, sp->radius, s->sp.b, s->sp.c);
        const uint32_t side = (uint32_t)std::ceil(2.0f * sp->radius);            // 1 .. 4
        s->accum_clamp = accum_clamp_for(samples_per_pixel * side * side);
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, s->sums, (size_t)width * height * 4u * sizeof(unsigned long long));
        handle_alloc(r, s->counters, SPLAT_COUNTER_BYTES);
        if (r != VK_OK) return r;
        for (Event &e : s->ev) if ((r = e.create()) != VK_OK) return r;
        if ((r = splat_zero(s.get())) != VK_OK) return r;
        *out = s.release();
        return VK_OK;
    });
}

int vk_splat_deposit(vk_splat *s, vk_paths *batch, const float *positions) {
    return guarded([&]() -> int {
        if (!s || !batch) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or path batch)");
        if (batch->scene != s->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the accumulator");
        if (!batch->begun) return fail(VK_ERR_BAD_ARG, "vk_splat_deposit before vk_paths_begin or vk_film_emit");
        if (batch->regen) return fail(VK_ERR_BAD_ARG, "vk_splat_deposit on a regenerating path batch (its results are not kept)");
        if (batch->live != 0u) return fail(VK_ERR_BAD_ARG, "the path batch has live paths (step or cull them first)");
        if (batch->splatted) return fail(VK_ERR_BAD_ARG, "the path batch has been deposited into an accumulator since its last begin or emit");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const uint64_t n = batch->started;
        if (n != 0u && positions) {
            const size_t floats = (size_t)n * 2u;
            if (floats > s->positions_cap) {
                DeviceBuffer<float> grown;
                int rc = VK_OK;
                handle_alloc(rc, grown, floats * sizeof(float));
                if (rc != VK_OK) return rc;
                s->positions = std::move(grown);
                s->positions_cap = floats;
            }
            HIP_TRY(hipMemcpy(s->positions, positions, floats * sizeof(float), hipMemcpyHostToDevice));
        }
        HIP_TRY(hipEventRecord(s->ev[0], nullptr));
        if (n != 0u) {
            SplatDepositArgs A;
            memset(&A, 0, sizeof(A));
            A.result_state = reinterpret_cast<const uint4 *>(batch->result_state.get()); A.result_status = batch->result_status;
            A.positions = positions ? reinterpret_cast<const float2 *>(s->positions.get()) : nullptr;
            A.sums = s->sums; A.counters = s->counters;
            A.P = s->filter;
            A.n = (uint32_t)n; A.width = s->width; A.height = s->height;
            A.accum_clamp = s->accum_clamp;
            launch_splat_deposit(A, s->tiled);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(s->ev[1], nullptr));
        s->timed[0] = true;
        s->deposits++;
        batch->splatted = true;
        return VK_OK;
    });
}

int vk_splat_resolve(vk_splat *s, float *rgb_out) {
    return guarded([&]() -> int {
        if (!s || !rgb_out) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or rgb_out)");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const size_t bytes = (size_t)s->width * s->height * 3u * sizeof(float);
        if (!s->out) {
            int rc = VK_OK;
            handle_alloc(rc, s->out, bytes);
            if (rc != VK_OK) return rc;
        }
        SplatResolveArgs A;
        memset(&A, 0, sizeof(A));
        A.sums = reinterpret_cast<const long long *>(s->sums.get()); A.out = s->out; A.n_pixels = s->width * s->height;
        HIP_TRY(hipEventRecord(s->ev[2], nullptr));
        launch_splat_resolve(A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s->ev[3], nullptr));
        s->timed[1] = true;
        HIP_TRY(hipMemcpy(rgb_out, s->out, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_splat_reset(vk_splat *s) {
    if (!s) return fail(VK_ERR_BAD_ARG, "null accumulator");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        return splat_zero(s);
    });
}

int vk_splat_get_info(vk_splat *s, vk_splat_info *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        std::vector<unsigned long long> stripes((size_t)SPLAT_STRIPES * SPLAT_STRIPE_WORDS);
        HIP_TRY(hipMemcpy(stripes.data(), s->counters, SPLAT_COUNTER_BYTES, hipMemcpyDeviceToHost));      // (waits for the null stream)
        unsigned long long c[SPLAT_COUNTERS] = {0ull, 0ull, 0ull, 0ull, 0ull};
        for (uint32_t k = 0; k < SPLAT_STRIPES; k++)
            for (uint32_t j = 0; j < SPLAT_COUNTERS; j++) c[j] += stripes[(size_t)k * SPLAT_STRIPE_WORDS + j];
        memset(out, 0, sizeof(*out));
        out->width = s->width; out->height = s->height; out->samples_per_pixel = s->spp; out->filter = s->sp.filter;
        out->deposited = c[0]; out->dropped = c[1]; out->clamped = c[2]; out->skipped = c[3];
        out->deposits = s->deposits; out->contributions = c[4];
        return VK_OK;
    });
}

void vk_splat_destroy(vk_splat *s) {
    if (s) splat_free(s);
}

// test hook (vecchio_amd_debug.h): the raw sums
int vk_debug_splat_sums(vk_splat *s, int64_t *sums4) {
    if (!s || !sums4) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or sums4)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        HIP_TRY(hipMemcpy(sums4, s->sums, (size_t)s->width * s->height * 4u * sizeof(int64_t), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the deposit's form from the next vk_splat_deposit on
int vk_debug_splat_form(vk_splat *s, uint32_t form) {
    if (!s) return fail(VK_ERR_BAD_ARG, "null accumulator");
    if (form > (uint32_t)VK_DEBUG_SPLAT_FORM_TILED) return fail(VK_ERR_BAD_ARG, "unknown deposit form");
    s->tiled = form == (uint32_t)VK_DEBUG_SPLAT_FORM_DEFAULT ? SPLAT_DEFAULT_TILED : form == (uint32_t)VK_DEBUG_SPLAT_FORM_TILED;
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the last deposit and resolve, from the events recorded around each; 0 for one not yet run
int vk_debug_splat_last_ms(vk_splat *s, double ms[2]) {
    if (!s || !ms) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        double got[2] = {0.0, 0.0};
        for (int k = 0; k < 2; k++) {
            if (!s->timed[k]) continue;
            HIP_TRY(hipEventSynchronize(s->ev[2 * k + 1]));
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, s->ev[2 * k], s->ev[2 * k + 1]));
            got[k] = (double)t;
        }
        for (int k = 0; k < 2; k++) ms[k] = got[k];
        return VK_OK;
    });
}

}  // extern "C"

// ---- robust film (vk_robust_*): a frame's fixed-point sums kept in K buckets per pixel — r, g, b and the count per bucket — on the scene's
// device (devices[0] of a multi-device scene).  robust_deposit_kernel adds a finished batch, robust_resolve_kernel<K> orders, trims and
// divides (vk_robust.hip); all on the null stream, on buffers and events the handle owns.  Of the batch a deposit reads its results and
// sets its `bucketed` flag; nothing of the scene handle is read but its device.
struct vk_robust {
    vk_scene *scene = nullptr;                      // as handed to vk_robust_create
    uint32_t width = 0, height = 0, spp = 0;
    vk_robust_params rp{};
    float accum_clamp = 0.0f;
    DeviceBuffer<unsigned long long> sums;          // [width * height][buckets][4], two's complement
    DeviceBuffer<unsigned long long> counters;      // deposited, dropped, clamped, skipped, in SPLAT_STRIPES stripes
    DeviceBuffer<float> out;                        // the resolved frame and its standard error on their way to the host (first resolve)
    Event ev[4];                                    // around the last deposit and resolve
    bool timed[2] = {false, false};
    uint64_t deposits = 0;
};

namespace {

void robust_free(vk_robust *s) {
    (void)hipSetDevice(first_part(s->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a deposit may still run)
    (void)hipGetLastError();
    delete s;
}

size_t robust_words(const vk_robust *s) { return (size_t)s->width * s->height * s->rp.buckets * 4u; }

int robust_zero(vk_robust *s) {
    HIP_TRY(hipMemsetAsync(s->sums, 0, robust_words(s) * sizeof(unsigned long long), nullptr));
    HIP_TRY(hipMemsetAsync(s->counters, 0, SPLAT_COUNTER_BYTES, nullptr));
    s->deposits = 0u;
    return VK_OK;
}

const char *robust_refusal(const vk_robust_params &rp) {
    if (rp.mode != VK_ROBUST_MEAN && rp.mode != VK_ROBUST_TRIM && rp.mode != VK_ROBUST_GINI) return "unknown mode";
    if (rp._pad != 0u) return "_pad must be 0";
    return nullptr;
}

}  // namespace

extern "C" {

int vk_robust_default_params(vk_robust_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    out->buckets = 8u; out->mode = VK_ROBUST_GINI; out->trim = 0u; out->_pad = 0u;
    return VK_OK;
}

int vk_robust_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, const vk_robust_params *rp, vk_robust **out) {
    if (!scene || !rp || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene, params or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if (rp->buckets < ROBUST_MIN_BUCKETS || rp->buckets > ROBUST_MAX_BUCKETS) return fail(VK_ERR_BAD_ARG, "buckets must be in 2..16");
    // (width * height < 2^64, and the product with buckets is taken only once that is below 2^27)
    if ((uint64_t)width * height > ROBUST_MAX_CELLS || (uint64_t)width * height * rp->buckets > ROBUST_MAX_CELLS)
        return fail(VK_ERR_BAD_ARG, "width * height * buckets exceeds 2^27");
    if (samples_per_pixel == 0u || samples_per_pixel > (1u << 26)) return fail(VK_ERR_BAD_ARG, "samples_per_pixel must be in 1..2^26");
    if (const char *why = robust_refusal(*rp)) return fail(VK_ERR_BAD_ARG, why);
    return guarded([&]() -> int {
        std::unique_ptr<vk_robust, void (*)(vk_robust *)> s(new vk_robust(), robust_free);
        s->scene = scene; s->width = width; s->height = height; s->spp = samples_per_pixel; s->rp = *rp;
        if (rp->mode != VK_ROBUST_TRIM) s->rp.trim = 0u;
        s->accum_clamp = accum_clamp_for(samples_per_pixel);
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, s->sums, robust_words(s.get()) * sizeof(unsigned long long));
        handle_alloc(r, s->counters, SPLAT_COUNTER_BYTES);
        if (r != VK_OK) return r;
        for (Event &e : s->ev) if ((r = e.create()) != VK_OK) return r;
        if ((r = robust_zero(s.get())) != VK_OK) return r;
        *out = s.release();
        return VK_OK;
    });
}

int vk_robust_deposit(vk_robust *s, vk_paths *batch) {
    return guarded([&]() -> int {
        if (!s || !batch) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or path batch)");
        if (batch->scene != s->scene) return fail(VK_ERR_BAD_ARG, "the path batch belongs to another scene than the accumulator");
        if (!batch->begun) return fail(VK_ERR_BAD_ARG, "vk_robust_deposit before vk_paths_begin or vk_film_emit");
        if (batch->regen) return fail(VK_ERR_BAD_ARG, "vk_robust_deposit on a regenerating path batch (its results are not kept)");
        if (batch->live != 0u) return fail(VK_ERR_BAD_ARG, "the path batch has live paths (step or cull them first)");
        if (batch->bucketed) return fail(VK_ERR_BAD_ARG, "the path batch has been deposited into a robust accumulator since its last begin or emit");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const uint64_t n = batch->started;
        HIP_TRY(hipEventRecord(s->ev[0], nullptr));
        if (n != 0u) {
            RobustDepositArgs A;
            memset(&A, 0, sizeof(A));
            A.result_state = reinterpret_cast<const uint4 *>(batch->result_state.get()); A.result_status = batch->result_status;
            A.sums = s->sums; A.counters = s->counters;
            A.n = (uint32_t)n; A.n_pixels = s->width * s->height; A.buckets = s->rp.buckets;
            A.accum_clamp = s->accum_clamp;
            launch_robust_deposit(A);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(s->ev[1], nullptr));
        s->timed[0] = true;
        s->deposits++;
        batch->bucketed = true;
        return VK_OK;
    });
}

int vk_robust_resolve(vk_robust *s, const vk_robust_params *how, float *rgb_out, float *stderr3_out) {
    return guarded([&]() -> int {
        if (!s || !rgb_out) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or rgb_out)");
        vk_robust_params rp = s->rp;
        if (how) {
            if (how->buckets != 0u && how->buckets != s->rp.buckets) return fail(VK_ERR_BAD_ARG, "how->buckets must be 0 or the accumulator's");
            if (const char *why = robust_refusal(*how)) return fail(VK_ERR_BAD_ARG, why);
            rp.mode = how->mode; rp.trim = how->mode == VK_ROBUST_TRIM ? how->trim : 0u;
        }
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const size_t floats = (size_t)s->width * s->height * 3u;
        if (!s->out) {
            int rc = VK_OK;
            handle_alloc(rc, s->out, 2u * floats * sizeof(float));
            if (rc != VK_OK) return rc;
        }
        RobustResolveArgs A;
        memset(&A, 0, sizeof(A));
        A.sums = reinterpret_cast<const RobustCell *>(s->sums.get()); A.rgb = s->out; A.se = stderr3_out ? s->out.get() + floats : nullptr;
        A.n_pixels = s->width * s->height; A.mode = rp.mode; A.trim = rp.trim;
        HIP_TRY(hipEventRecord(s->ev[2], nullptr));
        launch_robust_resolve(A, s->rp.buckets);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s->ev[3], nullptr));
        s->timed[1] = true;
        HIP_TRY(hipMemcpy(rgb_out, s->out, floats * sizeof(float), hipMemcpyDeviceToHost));
        if (stderr3_out) HIP_TRY(hipMemcpy(stderr3_out, s->out.get() + floats, floats * sizeof(float), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_robust_reset(vk_robust *s) {
    if (!s) return fail(VK_ERR_BAD_ARG, "null accumulator");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        return robust_zero(s);
    });
}

int vk_robust_get_info(vk_robust *s, vk_robust_info *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        std::vector<unsigned long long> stripes((size_t)SPLAT_STRIPES * SPLAT_STRIPE_WORDS);
        HIP_TRY(hipMemcpy(stripes.data(), s->counters, SPLAT_COUNTER_BYTES, hipMemcpyDeviceToHost));      // (waits for the null stream)
        unsigned long long c[ROBUST_COUNTERS] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t k = 0; k < SPLAT_STRIPES; k++)
            for (uint32_t j = 0; j < ROBUST_COUNTERS; j++) c[j] += stripes[(size_t)k * SPLAT_STRIPE_WORDS + j];
        memset(out, 0, sizeof(*out));
        out->width = s->width; out->height = s->height; out->samples_per_pixel = s->spp; out->buckets = s->rp.buckets;
        out->deposited = c[0]; out->dropped = c[1]; out->clamped = c[2]; out->skipped = c[3];
        out->deposits = s->deposits;
        return VK_OK;
    });
}

void vk_robust_destroy(vk_robust *s) {
    if (s) robust_free(s);
}

// test hook (vecchio_amd_debug.h): the raw state, [(pixel * K + b) * 4 + c] — the device's own layout
int vk_debug_robust_sums(vk_robust *s, int64_t *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        HIP_TRY(hipMemcpy(out, s->sums, robust_words(s) * sizeof(int64_t), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the last deposit and resolve, from the events recorded around each; 0 for one not yet run
int vk_debug_robust_last_ms(vk_robust *s, double ms[2]) {
    if (!s || !ms) return fail(VK_ERR_BAD_ARG, "null argument (accumulator or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        double got[2] = {0.0, 0.0};
        for (int k = 0; k < 2; k++) {
            if (!s->timed[k]) continue;
            HIP_TRY(hipEventSynchronize(s->ev[2 * k + 1]));
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, s->ev[2 * k], s->ev[2 * k + 1]));
            got[k] = (double)t;
        }
        for (int k = 0; k < 2; k++) ms[k] = got[k];
        return VK_OK;
    });
}

}  // extern "C"

// ---- light-path layers (vk_lpe_*): a tag per path id, kept up to date by lpe_record_kernel behind every bounce of vk_lpe_step, and a
// frame's fixed-point sums kept per pixel and layer — lpe_deposit_kernel adds a finished batch by the class of each result,
// lpe_resolve_kernel divides (vk_lpe.hip); all on the null stream of the scene's device (devices[0] of a multi-device scene), on buffers
// and events the handle owns.  Of the batch a step runs paths_bounce as vk_paths_step does and reads the bounce's records, hits and
// ids; a deposit reads its results and sets its `layered` flag.  Nothing of the scene handle is read but its device.
struct vk_lpe {
    vk_scene *scene = nullptr;                      // as handed to vk_lpe_create
    uint32_t width = 0, height = 0, spp = 0;
    uint64_t capacity = 0;
    uint32_t n_layers = 0, rest_layer = 0, n_rules = 0;
    LpeRule rules[LPE_MAX_RULES] = {};
    float accum_clamp = 0.0f;
    DeviceBuffer<uint32_t> tags;                    // [capacity][2]: sig, term
    DeviceBuffer<unsigned long long> sums;          // [width * height][n_layers][4], two's complement
    DeviceBuffer<unsigned long long> counters;      // deposited, dropped, clamped, skipped, in SPLAT_STRIPES stripes
    DeviceBuffer<float> out;                        // the resolved layer and its share on their way to the host (first resolve)
    Event ev[8];                                    // around the last record, deposit and resolve; [6], [7]: the record before the last
    bool timed[3] = {false, false, false};
    int rec_pair = 0;                               // the last record's events: ev[0], ev[1] (0) or ev[6], ev[7] (1)
    uint64_t deposits = 0, recorded = 0;            // accepted deposits; path-bounces recorded
    // the binding: the batch and the begin the tags describe, and how many of its bounces they hold (host state only)
    const vk_paths *bound = nullptr;                // for the identity check only
    uint64_t bound_begin = 0;
    uint32_t bound_bounces = 0;
};

namespace {

void lpe_free(vk_lpe *s) {
    (void)hipSetDevice(first_part(s->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a record or a deposit may still run)
    (void)hipGetLastError();
    delete s;
}

size_t lpe_words(const vk_lpe *s) { return (size_t)s->width * s->height * s->n_layers * 4u; }

int lpe_zero(vk_lpe *s) {
    HIP_TRY(hipMemsetAsync(s->sums, 0, lpe_words(s) * sizeof(unsigned long long), nullptr));
    HIP_TRY(hipMemsetAsync(s->counters, 0, SPLAT_COUNTER_BYTES, nullptr));
    s->deposits = 0u;
    return VK_OK;
}

const char *lpe_rule_refusal(const vk_lpe_rule &r, uint32_t n_layers) {
    if ((r.sig_value & ~r.sig_mask) != 0u) return "a rule's sig_value has bits outside its sig_mask";
    if (r.status_mask == 0u || (r.status_mask & ~LPE_STATUS_BITS) != 0u) return "a rule's status_mask must name MISS, ENDED or CULLED and nothing else";
    if (r.depth_min > r.depth_max) return "a rule's depth_min exceeds its depth_max";
    if (r.layer >= n_layers) return "a rule's layer is not below n_layers";
    if (r._pad != 0u) return "a rule's _pad must be 0";
    return nullptr;
}

bool lpe_bound_to(const vk_lpe *s, const vk_paths *batch) { return s->bound == batch && s->bound_begin == batch->begins; }

// what vk_lpe_step, vk_lpe_tags, vk_lpe_deposit and vk_debug_lpe_set_tags ask of any batch (nullptr: fine)
const char *lpe_batch_refusal(const vk_lpe *s, const vk_paths *batch, const char *who) {
    static thread_local std::string words;
    if (batch->scene != s->scene) words = "the path batch belongs to another scene than the tracker";
    else if (!batch->begun) words = std::string(who) + " before vk_paths_begin or vk_film_emit";
    else if (batch->regen) words = std::string(who) + " on a regenerating path batch (its results are not kept)";
    else if (batch->started > s->capacity) words = "the path batch has started more paths than the tracker's capacity";
    else return nullptr;
    return words.c_str();
}

}  // namespace

extern "C" {

int vk_lpe_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, uint64_t capacity, const vk_lpe_params *lp,
                  vk_lpe **out) {
    if (!scene || !lp || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene, params or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if (lp->n_layers < 1u || lp->n_layers > LPE_MAX_LAYERS) return fail(VK_ERR_BAD_ARG, "n_layers must be in 1..16");
    // (width * height < 2^64, and the product with n_layers is taken only once that is below 2^27)
    if ((uint64_t)width * height > LPE_MAX_CELLS || (uint64_t)width * height * lp->n_layers > LPE_MAX_CELLS)
        return fail(VK_ERR_BAD_ARG, "width * height * n_layers exceeds 2^27");
    if (samples_per_pixel == 0u || samples_per_pixel > (1u << 26)) return fail(VK_ERR_BAD_ARG, "samples_per_pixel must be in 1..2^26");
    if (capacity < 1u || capacity > PATHS_MAX) return fail(VK_ERR_BAD_ARG, "capacity must be in 1..2^24");
    if (lp->rest_layer >= lp->n_layers) return fail(VK_ERR_BAD_ARG, "rest_layer is not below n_layers");
    if (lp->n_rules > LPE_MAX_RULES) return fail(VK_ERR_BAD_ARG, "n_rules must be in 0..32");
    if (lp->n_rules > 0u && !lp->rules) return fail(VK_ERR_BAD_ARG, "null rules with n_rules > 0");
    if (lp->_pad != 0u) return fail(VK_ERR_BAD_ARG, "_pad must be 0");
    for (uint32_t k = 0; k < lp->n_rules; k++)
        if (const char *why = lpe_rule_refusal(lp->rules[k], lp->n_layers)) return fail(VK_ERR_BAD_ARG, why);
    return guarded([&]() -> int {
        std::unique_ptr<vk_lpe, void (*)(vk_lpe *)> s(new vk_lpe(), lpe_free);
        s->scene = scene; s->width = width; s->height = height; s->spp = samples_per_pixel; s->capacity = capacity;
        s->n_layers = lp->n_layers; s->rest_layer = lp->rest_layer; s->n_rules = lp->n_rules;
        static_assert(sizeof(LpeRule) == sizeof(vk_lpe_rule), "one rule, two names");
        for (uint32_t k = 0; k < lp->n_rules; k++) memcpy(&s->rules[k], &lp->rules[k], sizeof(LpeRule));
        s->accum_clamp = accum_clamp_for(samples_per_pixel);
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, s->tags, (size_t)capacity * 8u);
        handle_alloc(r, s->sums, lpe_words(s.get()) * sizeof(unsigned long long));
        handle_alloc(r, s->counters, SPLAT_COUNTER_BYTES);
        if (r != VK_OK) return r;
        for (Event &e : s->ev) if ((r = e.create()) != VK_OK) return r;
        HIP_TRY(hipMemsetAsync(s->tags, 0, (size_t)capacity * 8u, nullptr));
        if ((r = lpe_zero(s.get())) != VK_OK) return r;
        *out = s.release();
        return VK_OK;
    });
}

int vk_lpe_step(vk_lpe *s, vk_paths *p, uint32_t max_bounces, vk_paths_step_info *info) {
    return guarded([&]() -> int {
        if (!s || !p) return fail(VK_ERR_BAD_ARG, "null argument (tracker or path batch)");
        if (const char *why = lpe_batch_refusal(s, p, "vk_lpe_step")) return fail(VK_ERR_BAD_ARG, why);
        if (max_bounces == 0u) return fail(VK_ERR_BAD_ARG, "max_bounces must be >= 1");
        if (p->bounces != 0u) {
            if (!lpe_bound_to(s, p)) return fail(VK_ERR_BAD_ARG, "the path batch has run bounces and the tracker is not bound to it (bind with a step at bounce 0)");
            if (s->bound_bounces != p->bounces) return fail(VK_ERR_BAD_ARG, "the path batch has run bounces the tracker did not record (vk_paths_step in between)");
        }
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(p->scene);
        HIP_TRY(hipSetDevice(q->device));
        if (p->bounces == 0u) {
            // bind: the tags of this begin's ids start as "no bounce recorded"
            if (p->started != 0u) HIP_TRY(hipMemsetAsync(s->tags, 0, (size_t)p->started * 8u, nullptr));
            s->bound = p; s->bound_begin = p->begins; s->bound_bounces = 0u;
        }
        BounceTally T{};
        // a record's time is read behind the NEXT bounce's counts, which have waited for it: two pairs of events take turns, and only
        // the last record of the call is waited for
        bool pending = false;
        const auto record_ms = [&](int pair, double &ms_out) -> int {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev[pair ? 6 : 0], s->ev[pair ? 7 : 1]));
            ms_out += (double)ms;
            return VK_OK;
        };
        while (p->live != 0u && T.bounces < max_bounces) {
            const uint64_t n = p->live;
            const uint32_t bounce = p->bounces;
            HIP_TRY(hipEventRecord(p->ev0, nullptr));
            int rc = paths_bounce(p, q, nullptr, T);
            if (rc != VK_OK) return rc;
            if (pending && (rc = record_ms(s->rec_pair, T.kernel_ms)) != VK_OK) return rc;
            // the bounce's records, hits and ids are where the compaction read them: shaded[0, n), hits[0, n), ids[cur ^ 1][0, n)
            LpeRecordArgs A;
            memset(&A, 0, sizeof(A));
            A.shaded = reinterpret_cast<const uint4 *>(p->shaded.get()); A.hits = reinterpret_cast<const uint4 *>(p->hits.get());
            A.ids = p->ids[p->cur ^ 1u]; A.tags = reinterpret_cast<uint2 *>(s->tags.get());
            A.n = (uint32_t)n; A.capacity = (uint32_t)s->capacity; A.bounce = bounce;
            const int pair = pending ? s->rec_pair ^ 1 : 0;
            HIP_TRY(hipEventRecord(s->ev[pair ? 6 : 0], nullptr));
            launch_lpe_record(A);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(s->ev[pair ? 7 : 1], nullptr));
            s->rec_pair = pair; pending = true; s->timed[0] = true;
            T.launches++;
            s->bound_bounces = p->bounces;
            s->recorded += n;
        }
        if (pending) {
            HIP_TRY(hipEventSynchronize(s->ev[s->rec_pair ? 7 : 1]));
            int rc = record_ms(s->rec_pair, T.kernel_ms);
            if (rc != VK_OK) return rc;
        }
        vk_paths_step_info I;
        memset(&I, 0, sizeof(I));
        I.traced = T.traced; I.missed = T.missed; I.ended = T.ended; I.bad = T.bad;
        I.bounces = T.bounces; I.kernel_launches = T.launches; I.kernel_ms = T.kernel_ms;
        I.live = p->live;
        I.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = I;
        return VK_OK;
    });
}

int vk_lpe_tags(vk_lpe *s, vk_paths *p, uint32_t *sig, uint32_t *term) {
    return guarded([&]() -> int {
        if (!s || !p) return fail(VK_ERR_BAD_ARG, "null argument (tracker or path batch)");
        if (const char *why = lpe_batch_refusal(s, p, "vk_lpe_tags")) return fail(VK_ERR_BAD_ARG, why);
        if (!lpe_bound_to(s, p)) return fail(VK_ERR_BAD_ARG, "the tracker is not bound to the path batch");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const size_t n = (size_t)p->started;
        if (n == 0u || (!sig && !term)) { HIP_TRY(hipStreamSynchronize(nullptr)); return VK_OK; }
        std::vector<uint32_t> both(2u * n);
        HIP_TRY(hipMemcpy(both.data(), s->tags, n * 8u, hipMemcpyDeviceToHost));      // (waits for the null stream)
        for (size_t i = 0; i < n; i++) {
            if (sig) sig[i] = both[2u * i];
            if (term) term[i] = both[2u * i + 1u];
        }
        return VK_OK;
    });
}

int vk_lpe_deposit(vk_lpe *s, vk_paths *batch) {
    return guarded([&]() -> int {
        if (!s || !batch) return fail(VK_ERR_BAD_ARG, "null argument (tracker or path batch)");
        if (const char *why = lpe_batch_refusal(s, batch, "vk_lpe_deposit")) return fail(VK_ERR_BAD_ARG, why);
        if (batch->live != 0u) return fail(VK_ERR_BAD_ARG, "the path batch has live paths (step or cull them first)");
        if (batch->layered) return fail(VK_ERR_BAD_ARG, "the path batch has been deposited into a layer accumulator since its last begin or emit");
        if (!lpe_bound_to(s, batch)) return fail(VK_ERR_BAD_ARG, "the tracker is not bound to the path batch");
        if (s->bound_bounces != batch->bounces) return fail(VK_ERR_BAD_ARG, "the path batch has run bounces the tracker did not record (vk_paths_step in between)");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const uint64_t n = batch->started;
        HIP_TRY(hipEventRecord(s->ev[2], nullptr));
        if (n != 0u) {
            LpeDepositArgs A;
            memset(&A, 0, sizeof(A));
            A.result_state = reinterpret_cast<const uint4 *>(batch->result_state.get()); A.result_status = batch->result_status;
            A.tags = reinterpret_cast<const uint2 *>(s->tags.get());
            A.sums = s->sums; A.counters = s->counters;
            A.n = (uint32_t)n; A.n_pixels = s->width * s->height; A.n_layers = s->n_layers; A.rest_layer = s->rest_layer; A.n_rules = s->n_rules;
            A.accum_clamp = s->accum_clamp;
            for (uint32_t k = 0; k < s->n_rules; k++) A.rules[k] = s->rules[k];
            launch_lpe_deposit(A);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(s->ev[3], nullptr));
        s->timed[1] = true;
        s->deposits++;
        batch->layered = true;
        return VK_OK;
    });
}

int vk_lpe_resolve(vk_lpe *s, uint32_t layer, uint32_t n, float *rgb_out, float *share_out) {
    return guarded([&]() -> int {
        if (!s || !rgb_out) return fail(VK_ERR_BAD_ARG, "null argument (tracker or rgb_out)");
        if (layer != VK_LPE_ALL && layer >= s->n_layers) return fail(VK_ERR_BAD_ARG, "layer must be below n_layers or VK_LPE_ALL");
        if (n == 0u) return fail(VK_ERR_BAD_ARG, "n must be >= 1");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        const size_t px = (size_t)s->width * s->height;
        if (!s->out) {
            int rc = VK_OK;
            handle_alloc(rc, s->out, 4u * px * sizeof(float));
            if (rc != VK_OK) return rc;
        }
        LpeResolveArgs A;
        memset(&A, 0, sizeof(A));
        A.sums = reinterpret_cast<const long long *>(s->sums.get()); A.rgb = s->out; A.share = share_out ? s->out.get() + 3u * px : nullptr;
        A.n_pixels = (uint32_t)px; A.n_layers = s->n_layers; A.layer = layer; A.n = (float)n;
        HIP_TRY(hipEventRecord(s->ev[4], nullptr));
        launch_lpe_resolve(A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s->ev[5], nullptr));
        s->timed[2] = true;
        HIP_TRY(hipMemcpy(rgb_out, s->out, 3u * px * sizeof(float), hipMemcpyDeviceToHost));
        if (share_out) HIP_TRY(hipMemcpy(share_out, s->out.get() + 3u * px, px * sizeof(float), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_lpe_reset(vk_lpe *s) {
    if (!s) return fail(VK_ERR_BAD_ARG, "null tracker");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        return lpe_zero(s);
    });
}

int vk_lpe_get_info(vk_lpe *s, vk_lpe_info *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument (tracker or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        std::vector<unsigned long long> stripes((size_t)SPLAT_STRIPES * SPLAT_STRIPE_WORDS);
        HIP_TRY(hipMemcpy(stripes.data(), s->counters, SPLAT_COUNTER_BYTES, hipMemcpyDeviceToHost));      // (waits for the null stream)
        unsigned long long c[LPE_COUNTERS] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t k = 0; k < SPLAT_STRIPES; k++)
            for (uint32_t j = 0; j < LPE_COUNTERS; j++) c[j] += stripes[(size_t)k * SPLAT_STRIPE_WORDS + j];
        memset(out, 0, sizeof(*out));
        out->width = s->width; out->height = s->height; out->samples_per_pixel = s->spp; out->n_layers = s->n_layers;
        out->rest_layer = s->rest_layer; out->n_rules = s->n_rules; out->capacity = s->capacity;
        out->deposited = c[0]; out->dropped = c[1]; out->clamped = c[2]; out->skipped = c[3];
        out->deposits = s->deposits; out->recorded = s->recorded;
        return VK_OK;
    });
}

void vk_lpe_destroy(vk_lpe *s) {
    if (s) lpe_free(s);
}

// test hook (vecchio_amd_debug.h): the raw state, [(pixel * n_layers + l) * 4 + c] — the device's own layout
int vk_debug_lpe_sums(vk_lpe *s, int64_t *out) {
    if (!s || !out) return fail(VK_ERR_BAD_ARG, "null argument (tracker or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        HIP_TRY(hipMemcpy(out, s->sums, lpe_words(s) * sizeof(int64_t), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the tags of the batch's started ids from the host, and the tracker bound to the batch as if it had
// recorded every bounce the batch has run
int vk_debug_lpe_set_tags(vk_lpe *s, vk_paths *batch, const uint32_t *sig, const uint32_t *term) {
    return guarded([&]() -> int {
        if (!s || !batch) return fail(VK_ERR_BAD_ARG, "null argument (tracker or path batch)");
        if (const char *why = lpe_batch_refusal(s, batch, "vk_debug_lpe_set_tags")) return fail(VK_ERR_BAD_ARG, why);
        const size_t n = (size_t)batch->started;
        if (n != 0u && (!sig || !term)) return fail(VK_ERR_BAD_ARG, "null sig or term with started paths");
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        if (n != 0u) {
            std::vector<uint32_t> both(2u * n);
            for (size_t i = 0; i < n; i++) { both[2u * i] = sig[i]; both[2u * i + 1u] = term[i]; }
            HIP_TRY(hipMemcpy(s->tags, both.data(), n * 8u, hipMemcpyHostToDevice));
        }
        s->bound = batch; s->bound_begin = batch->begins; s->bound_bounces = batch->bounces;
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the last record, deposit and resolve, from the events recorded around each; 0 for one not yet run
int vk_debug_lpe_last_ms(vk_lpe *s, double ms[3]) {
    if (!s || !ms) return fail(VK_ERR_BAD_ARG, "null argument (tracker or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(s->scene)->device));
        double got[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; k++) {
            if (!s->timed[k]) continue;
            const int a = k == 0 && s->rec_pair ? 6 : 2 * k, b = a + 1;
            HIP_TRY(hipEventSynchronize(s->ev[b]));
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, s->ev[a], s->ev[b]));
            got[k] = (double)t;
        }
        for (int k = 0; k < 3; k++) ms[k] = got[k];
        return VK_OK;
    });
}

}  // extern "C"

// ---- display transform (vk_tone_*): a frame on the scene's device (devices[0] of a multi-device scene), its luminance histogram
// (tone_meter_*_kernel), the exposure metered from it on the host (vk_tone_solve) and its encoding to 8-bit codes
// (tone_encode_kernel<curve, table, dither>, vk_tone.hip); all on the null stream, on buffers and events the handle owns.  Nothing of
// the scene handle is read but its device.
struct vk_tone {
    vk_scene *scene = nullptr;                      // as handed to vk_tone_create
    uint32_t width = 0, height = 0;
    DeviceBuffer<float> frame;                      // [width * height * 3], y up: vk_tone_load's staging buffer and the kernels' input
    DeviceBuffer<uint32_t> hist;                    // TONE_BINS bins, then TONE_COUNTERS 64-bit counters
    DeviceBuffer<float> tables;                     // sRGB's and gamma 2.2's thresholds, TONE_TABLE floats each
    DeviceBuffer<uint8_t> out;                      // the codes on their way to the host (first vk_tone_encode)
    Event ev[4];                                    // around the last meter and encode kernels
    bool timed[2] = {false, false};
    bool loaded = false, metered = false, has_prev = false;
    double log2_used = 0.0;                         // the last non-empty meter's (has_prev)
    float exposure = 1.0f;
    uint32_t form = TONE_FORM_LDS;
    uint64_t loads = 0, meters = 0, encodes = 0;
};

namespace {

void tone_free(vk_tone *t) {
    (void)hipSetDevice(first_part(t->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (an encode or a copy may still run)
    (void)hipGetLastError();
    delete t;
}

size_t tone_pixels(const vk_tone *t) { return (size_t)t->width * t->height; }

constexpr size_t TONE_HIST_BYTES = TONE_BINS * sizeof(uint32_t) + TONE_COUNTERS * sizeof(unsigned long long);

// the inverse of a transfer's encoding at c in [0, 1], in f64
double tone_inverse(uint32_t transfer, double c) {
    if (transfer == VK_TONE_TRANSFER_SRGB) return c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
    return std::pow(c, 2.2);
}

// H[j], j = 1 .. 510, into h[j - 1]: the smallest f32 not below inverse(j / 510)
void tone_table(uint32_t transfer, float h[TONE_TABLE]) {
    for (uint32_t j = 1; j <= TONE_TABLE; j++) {
        const double v = tone_inverse(transfer, (double)j / 510.0);
        float f = (float)v;
        if ((double)f < v) f = std::nextafterf(f, INFINITY);
        h[j - 1u] = f;
    }
}

// 2^e * (1 + f) for x = e + f, e = floor(x): the piecewise-linear exp2 of the float format, from basic operations (|x| <= 1000)
double tone_pexp2(double x) {
    long long e = (long long)x;
    if ((double)e > x) e -= 1;
    const double f = x - (double)e;
    return (1.0 + f) * vk::bits_f64((uint64_t)(e + 1023) << 52);
}

const char *tone_meter_refusal(const vk_tone_meter_params &mp) {
    if (mp._pad[0] != 0u || mp._pad[1] != 0u) return "_pad must be 0";
    if (!std::isfinite(mp.low_fraction) || !std::isfinite(mp.high_fraction) || mp.low_fraction < 0.0f || mp.high_fraction < 0.0f)
        return "low_fraction and high_fraction must be finite and >= 0";
    if ((double)mp.low_fraction + (double)mp.high_fraction >= 1.0) return "low_fraction + high_fraction must be below 1";
    if (!std::isfinite(mp.key) || !(mp.key > 0.0f)) return "key must be finite and > 0";
    if (!(mp.blend >= 0.0f && mp.blend <= 1.0f)) return "blend must be in 0..1";
    if (!std::isfinite(mp.min_log2) || !std::isfinite(mp.max_log2) || std::fabs(mp.min_log2) > 1000.0f || std::fabs(mp.max_log2) > 1000.0f)
        return "min_log2 and max_log2 must be finite and within -1000..1000";
    if (mp.min_log2 > mp.max_log2) return "min_log2 must not exceed max_log2";
    return nullptr;
}

const char *tone_refusal(const vk_tone_params &tp) {
    if (tp._pad != 0u) return "_pad must be 0";
    if (tp.curve > (uint32_t)VK_TONE_ACES) return "unknown curve";
    if (tp.transfer > (uint32_t)VK_TONE_TRANSFER_GAMMA22) return "unknown transfer";
    if (tp.flags & ~(uint32_t)(VK_TONE_USE_METERED | VK_TONE_DITHER)) return "unknown tone flags";
    if ((tp.flags & VK_TONE_DITHER) && tp.transfer == (uint32_t)VK_TONE_TRANSFER_REFERENCE) return "dither needs a table transfer (not the reference transfer)";
    if (!std::isfinite(tp.exposure) || !(tp.exposure > 0.0f)) return "exposure must be finite and > 0";
    const bool inf_ok = tp.curve == (uint32_t)VK_TONE_REINHARD && tp.white == INFINITY;
    if (!inf_ok && (!std::isfinite(tp.white) || !(tp.white > 0.0f))) return "white must be finite and > 0 (+inf with VK_TONE_REINHARD)";
    return nullptr;
}

// the encode of the handle's frame into d_out (4-byte aligned, the handle's device); the arguments have been checked
int enqueue_tone_encode(vk_tone *t, const vk_tone_params &tp, uint8_t *d_out) {
    ToneEncodeArgs A;
    memset(&A, 0, sizeof(A));
    const bool table = tp.transfer != (uint32_t)VK_TONE_TRANSFER_REFERENCE;
    A.rgb = t->frame; A.out = d_out; A.width = t->width; A.height = t->height;
    A.table = table ? t->tables.get() + (tp.transfer == (uint32_t)VK_TONE_TRANSFER_GAMMA22 ? TONE_TABLE : 0u) : nullptr;
    A.E = tp.exposure * ((tp.flags & VK_TONE_USE_METERED) ? t->exposure : 1.0f);
    A.p = tp.curve == (uint32_t)VK_TONE_REINHARD ? tp.white * tp.white : tp.curve == (uint32_t)VK_TONE_HABLE ? tone_hable(tp.white) : 0.0f;
    A.seed = tp.seed;
    HIP_TRY(hipEventRecord(t->ev[2], nullptr));
    launch_tone_encode(A, tp.curve, table, (tp.flags & VK_TONE_DITHER) != 0u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev[3], nullptr));
    t->timed[1] = true;
    t->encodes++;
    return VK_OK;
}

int check_tone_encode(vk_tone *t, const vk_tone_params *tp, const void *out) {
    if (!t || !tp || !out) return fail(VK_ERR_BAD_ARG, "null argument (tone handle, params or output)");
    if (const char *why = tone_refusal(*tp)) return fail(VK_ERR_BAD_ARG, why);
    if (!t->loaded) return fail(VK_ERR_BAD_ARG, "vk_tone_encode before vk_tone_load");
    if ((tp->flags & VK_TONE_USE_METERED) && !t->metered) return fail(VK_ERR_BAD_ARG, "VK_TONE_USE_METERED before vk_tone_meter");
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_tone_default_meter_params(vk_tone_meter_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->key = 0.18f; out->low_fraction = 0.10f; out->high_fraction = 0.02f; out->blend = 1.0f; out->min_log2 = -16.0f; out->max_log2 = 16.0f;
    return VK_OK;
}

int vk_tone_default_params(vk_tone_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->curve = VK_TONE_ACES; out->transfer = VK_TONE_TRANSFER_SRGB; out->flags = VK_TONE_USE_METERED;
    out->exposure = 1.0f; out->white = 11.2f; out->seed = 0u;
    return VK_OK;
}

int vk_tone_solve(const uint32_t bins[640], const vk_tone_meter_params *mp, const double *prev_log2, vk_tone_meter_info *out) {
    if (!bins || !mp || !out) return fail(VK_ERR_BAD_ARG, "null argument (bins, params or out)");
    if (const char *why = tone_meter_refusal(*mp)) return fail(VK_ERR_BAD_ARG, why);
    if (prev_log2 && !std::isfinite(*prev_log2)) return fail(VK_ERR_BAD_ARG, "prev_log2 must be finite");
    uint64_t N = 0u;
    for (uint32_t b = 0; b < TONE_BINS; b++) N += bins[b];
    const double lo = (double)mp->low_fraction * (double)N, hi = (1.0 - (double)mp->high_fraction) * (double)N;
    double S = 0.0, W = 0.0, c = 0.0;
    for (uint32_t b = 0; b < TONE_BINS; b++) {
        const double next = c + (double)bins[b];
        const double top = next < hi ? next : hi, bottom = c > lo ? c : lo;
        const double w = top - bottom > 0.0 ? top - bottom : 0.0;
        const double l = -20.0 + ((double)b + 0.5) / 16.0;
        S += w * l; W += w;
        c = next;
    }
    vk_tone_meter_info info;
    memset(&info, 0, sizeof(info));
    info.binned = N;
    const double mn = (double)mp->min_log2, mx = (double)mp->max_log2;
    if (N == 0u || !(W > 0.0)) {
        info.flags = VK_TONE_METER_EMPTY;
        if (prev_log2) {
            const double u = *prev_log2 < mn ? mn : (*prev_log2 > mx ? mx : *prev_log2);
            info.log2_target = *prev_log2; info.log2_used = u;
            info.exposure = (float)((double)mp->key * tone_pexp2(-u));
        } else {
            info.exposure = 1.0f;
        }
    } else {
        const double target = S / W;
        double u = prev_log2 ? *prev_log2 + (double)mp->blend * (target - *prev_log2) : target;
        u = u < mn ? mn : (u > mx ? mx : u);
        info.log2_target = target; info.log2_used = u;
        info.exposure = (float)((double)mp->key * tone_pexp2(-u));
    }
    *out = info;
    return VK_OK;
}

int vk_tone_create(vk_scene *scene, uint32_t width, uint32_t height, vk_tone **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if ((uint64_t)width * height > TONE_MAX_PIXELS) return fail(VK_ERR_BAD_ARG, "width * height exceeds 2^27");
    return guarded([&]() -> int {
        std::unique_ptr<vk_tone, void (*)(vk_tone *)> t(new vk_tone(), tone_free);
        t->scene = scene; t->width = width; t->height = height;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, t->frame, tone_pixels(t.get()) * 3u * sizeof(float));
        handle_alloc(r, t->hist, TONE_HIST_BYTES);
        handle_alloc(r, t->tables, 2u * TONE_TABLE * sizeof(float));
        if (r != VK_OK) return r;
        for (Event &e : t->ev) if ((r = e.create()) != VK_OK) return r;
        float h[2u * TONE_TABLE];
        tone_table(VK_TONE_TRANSFER_SRGB, h);
        tone_table(VK_TONE_TRANSFER_GAMMA22, h + TONE_TABLE);
        HIP_TRY(hipMemcpy(t->tables, h, sizeof(h), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(t->hist, 0, TONE_HIST_BYTES));
        *out = t.release();
        return VK_OK;
    });
}

int vk_tone_load(vk_tone *t, const float *rgb) {
    if (!t || !rgb) return fail(VK_ERR_BAD_ARG, "null argument (tone handle or rgb)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        float *const host[1] = {const_cast<float *>(rgb)};
        const uint32_t comps[1] = {3u};
        StagedImages im;
        int rc = im.upload(t->frame, host, comps, 1, tone_pixels(t), 0x1u);
        if (rc != VK_OK) return rc;
        t->loaded = true; t->loads++;
        return VK_OK;
    });
}

int vk_tone_load_device(vk_tone *t, const void *d_rgb) {
    if (!t || !d_rgb) return fail(VK_ERR_BAD_ARG, "null argument (tone handle or d_rgb)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        HIP_TRY(hipMemcpyAsync(t->frame, d_rgb, tone_pixels(t) * 3u * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        t->loaded = true; t->loads++;
        return VK_OK;
    });
}

int vk_tone_meter(vk_tone *t, const vk_tone_meter_params *mp, vk_tone_meter_info *out) {
    if (!t || !mp || !out) return fail(VK_ERR_BAD_ARG, "null argument (tone handle, params or out)");
    if (const char *why = tone_meter_refusal(*mp)) return fail(VK_ERR_BAD_ARG, why);
    if (!t->loaded) return fail(VK_ERR_BAD_ARG, "vk_tone_meter before vk_tone_load");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        ToneMeterArgs A;
        memset(&A, 0, sizeof(A));
        A.rgb = t->frame; A.bins = t->hist; A.counters = reinterpret_cast<unsigned long long *>(t->hist.get() + TONE_BINS);
        A.n_pixels = (uint32_t)tone_pixels(t);
        HIP_TRY(hipMemsetAsync(t->hist, 0, TONE_HIST_BYTES, nullptr));
        HIP_TRY(hipEventRecord(t->ev[0], nullptr));
        launch_tone_meter(A, t->form);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t->ev[1], nullptr));
        t->timed[0] = true;
        uint32_t host[TONE_HIST_BYTES / sizeof(uint32_t)];
        HIP_TRY(hipMemcpy(host, t->hist, TONE_HIST_BYTES, hipMemcpyDeviceToHost));      // (waits for the null stream)
        unsigned long long counters[TONE_COUNTERS];
        memcpy(counters, host + TONE_BINS, sizeof(counters));
        vk_tone_meter_info info;
        const int rc = vk_tone_solve(host, mp, t->has_prev ? &t->log2_used : nullptr, &info);
        if (rc != VK_OK) return rc;
        info.below = counters[TONE_BELOW]; info.above = counters[TONE_ABOVE]; info.nonfinite = counters[TONE_NONFINITE];
        if (!(info.flags & VK_TONE_METER_EMPTY)) { t->has_prev = true; t->log2_used = info.log2_used; }
        t->exposure = info.exposure; t->metered = true; t->meters++;
        *out = info;
        return VK_OK;
    });
}

int vk_tone_encode(vk_tone *t, const vk_tone_params *tp, uint8_t *rgb8_out) {
    int rc = check_tone_encode(t, tp, rgb8_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        const size_t bytes = tone_pixels(t) * 3u;
        if (!t->out) {
            int r = VK_OK;
            handle_alloc(r, t->out, bytes);
            if (r != VK_OK) return r;
        }
        int r = enqueue_tone_encode(t, *tp, t->out);
        if (r != VK_OK) return r;
        HIP_TRY(hipMemcpy(rgb8_out, t->out, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_tone_encode_device(vk_tone *t, const vk_tone_params *tp, void *d_rgb8_out) {
    int rc = check_tone_encode(t, tp, d_rgb8_out);
    if (rc != VK_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_rgb8_out) & 3u) return fail(VK_ERR_BAD_ARG, "d_rgb8_out must be 4-byte aligned");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        return enqueue_tone_encode(t, *tp, static_cast<uint8_t *>(d_rgb8_out));
    });
}

int vk_tone_reset(vk_tone *t) {
    if (!t) return fail(VK_ERR_BAD_ARG, "null tone handle");
    t->loaded = false; t->metered = false; t->has_prev = false; t->log2_used = 0.0; t->exposure = 1.0f;
    return VK_OK;
}

int vk_tone_get_info(vk_tone *t, vk_tone_info *out) {
    if (!t || !out) return fail(VK_ERR_BAD_ARG, "null argument (tone handle or out)");
    memset(out, 0, sizeof(*out));
    out->width = t->width; out->height = t->height; out->loads = t->loads; out->meters = t->meters; out->encodes = t->encodes;
    out->exposure = t->exposure; out->metered = t->metered ? 1u : 0u; out->log2_used = t->log2_used;
    return VK_OK;
}

void vk_tone_destroy(vk_tone *t) {
    if (t) tone_free(t);
}

// test hook (vecchio_amd_debug.h): the last meter's histogram and counters (zeros before the first)
int vk_debug_tone_histogram(vk_tone *t, uint32_t bins[640], uint64_t counters[4]) {
    if (!t || !bins || !counters) return fail(VK_ERR_BAD_ARG, "null argument (tone handle, bins or counters)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        uint32_t host[TONE_HIST_BYTES / sizeof(uint32_t)];
        HIP_TRY(hipMemcpy(host, t->hist, TONE_HIST_BYTES, hipMemcpyDeviceToHost));
        memcpy(bins, host, TONE_BINS * sizeof(uint32_t));
        memcpy(counters, host + TONE_BINS, TONE_COUNTERS * sizeof(uint64_t));
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): a table transfer's 510 thresholds, as every handle holds them; host code
int vk_debug_tone_table(uint32_t transfer, float out[510]) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (transfer != (uint32_t)VK_TONE_TRANSFER_SRGB && transfer != (uint32_t)VK_TONE_TRANSFER_GAMMA22)
        return fail(VK_ERR_BAD_ARG, "not a table transfer");
    tone_table(transfer, out);
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the meter kernel's form
int vk_debug_tone_set_form(vk_tone *t, uint32_t form) {
    if (!t) return fail(VK_ERR_BAD_ARG, "null tone handle");
    if (form != (uint32_t)VK_TONE_FORM_LDS && form != (uint32_t)VK_TONE_FORM_PLAIN) return fail(VK_ERR_BAD_ARG, "unknown meter form");
    t->form = form;
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the last meter and encode kernels, from the events recorded around each; 0 for one not yet run
int vk_debug_tone_last_ms(vk_tone *t, double ms[2]) {
    if (!t || !ms) return fail(VK_ERR_BAD_ARG, "null argument (tone handle or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(t->scene)->device));
        double got[2] = {0.0, 0.0};
        for (int k = 0; k < 2; k++) {
            if (!t->timed[k]) continue;
            HIP_TRY(hipEventSynchronize(t->ev[2 * k + 1]));
            float e = 0.0f;
            HIP_TRY(hipEventElapsedTime(&e, t->ev[2 * k], t->ev[2 * k + 1]));
            got[k] = (double)e;
        }
        for (int k = 0; k < 2; k++) ms[k] = got[k];
        return VK_OK;
    });
}

}  // extern "C"

// ---- non-local means (vk_nlm_*): a copy of the loaded images on the scene's device (devices[0] of a multi-device scene), the four planes
// nlm_prepare_kernel makes of it and the filter over them (nlm_filter_kernel<form, halo>, vk_nlm.hip); all on the null stream, on buffers
// and events the handle owns.  Nothing of the scene handle is read but its device.
struct vk_nlm {
    vk_scene *scene = nullptr;                      // as handed to vk_nlm_create
    uint32_t width = 0, height = 0;
    DeviceBuffer<float> raw;                        // color, stderr3, albedo as loaded: [3][width * height * 3]
    DeviceBuffer<float> planes;                     // I, V, Vf, a: [4][3][width * height]
    DeviceBuffer<float> out;                        // rgb_out and stderr3_out on their way to the host (first vk_nlm_filter)
    Event ev[4];                                    // around the last prepare and filter kernels
    bool timed[2] = {false, false};
    bool loaded = false, has_albedo = false;
    float floor_used = 1e-3f;                       // the albedo_floor the planes were prepared with
    uint32_t form = NLM_FORM_AUTO, last_form = 0u, last_launches = 0u;
    uint64_t loads = 0, filters = 0;
};

namespace {

void nlm_free(vk_nlm *h) {
    (void)hipSetDevice(first_part(h->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (a filter or a copy may still run)
    (void)hipGetLastError();
    delete h;
}

size_t nlm_pixels(const vk_nlm *h) { return (size_t)h->width * h->height; }

// Per (R, F) the form that was measured faster on the MI355X (tools/nlm_report.py, DESIGN.md "Non-local means"): with a patch (F >= 1:
// measured at (1, 1), (3, 1), (10, 1), (2, 2), (7, 2), (1, 3), (7, 3), (10, 3)) the tiled form, 2.5 to 11 times faster — the pairs of a
// patch are shared —; without one (F = 0) there is nothing to share and the plain form is level at R = 1 and 1.1 to 1.2 times faster
// at R = 10.  The gain follows F, not R, so R has no say.
uint32_t nlm_auto_form(uint32_t R, uint32_t F) {
    (void)R;
    return F == 0u ? NLM_FORM_PLAIN : NLM_FORM_TILED;
}

const char *nlm_refusal(const vk_nlm_params &p) {
    if (p.search_radius < 1u || p.search_radius > NLM_MAX_R) return "search_radius must be in 1..10";
    if (p.patch_radius > NLM_MAX_F) return "patch_radius must be in 0..3";
    if (!std::isfinite(p.k) || !(p.k > 0.0f)) return "k must be finite and > 0";
    if (!std::isfinite(p.alpha) || !(p.alpha >= 0.0f)) return "alpha must be finite and >= 0";
    if (!std::isfinite(p.albedo_floor) || !(p.albedo_floor > 0.0f)) return "albedo_floor must be finite and > 0";
    if (p.flags != 0u) return "unknown nlm flags";
    return nullptr;
}

// the prepare kernel over the handle's copy of the loaded images, into its planes
int enqueue_nlm_prepare(vk_nlm *h, float albedo_floor) {
    const size_t n = nlm_pixels(h);
    NlmPrepareArgs A;
    memset(&A, 0, sizeof(A));
    A.color = h->raw; A.stderr3 = h->raw.get() + 3u * n; A.albedo = h->has_albedo ? h->raw.get() + 6u * n : nullptr;
    A.I = h->planes; A.V = h->planes.get() + 3u * n; A.Vf = h->planes.get() + 6u * n; A.a = h->planes.get() + 9u * n;
    A.width = h->width; A.height = h->height; A.albedo_floor = albedo_floor;
    HIP_TRY(hipEventRecord(h->ev[0], nullptr));
    launch_nlm_prepare(A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], nullptr));
    h->timed[0] = true;
    h->floor_used = albedo_floor;
    return VK_OK;
}

// the filter of the handle's planes into d_out and d_se (may be null), on the handle's device; the arguments have been checked
int enqueue_nlm_filter(vk_nlm *h, const vk_nlm_params &p, float *d_out, float *d_se) {
    const size_t n = nlm_pixels(h);
    h->last_launches = 0u;
    if (h->has_albedo && p.albedo_floor != h->floor_used) {
        int rc = enqueue_nlm_prepare(h, p.albedo_floor);
        if (rc != VK_OK) return rc;
        h->last_launches++;
    }
    NlmFilterArgs A;
    memset(&A, 0, sizeof(A));
    A.P.I = h->planes; A.P.V = h->planes.get() + 3u * n; A.P.Vf = h->planes.get() + 6u * n; A.P.a = h->planes.get() + 9u * n;
    A.P.width = h->width; A.P.height = h->height;
    A.out = d_out; A.stderr3_out = d_se;
    A.R = (int)p.search_radius; A.F = (int)p.patch_radius;
    A.alpha = p.alpha; A.kk = p.k * p.k;
    const uint32_t form = h->form == NLM_FORM_AUTO ? nlm_auto_form(p.search_radius, p.patch_radius) : h->form;
    HIP_TRY(hipEventRecord(h->ev[2], nullptr));
    launch_nlm_filter(A, form);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], nullptr));
    h->timed[1] = true;
    h->last_form = form; h->last_launches++; h->filters++;
    return VK_OK;
}

int check_nlm_filter(vk_nlm *h, const vk_nlm_params *p, const void *out) {
    if (!h || !p || !out) return fail(VK_ERR_BAD_ARG, "null argument (nlm handle, params or output)");
    if (const char *why = nlm_refusal(*p)) return fail(VK_ERR_BAD_ARG, why);
    if (!h->loaded) return fail(VK_ERR_BAD_ARG, "vk_nlm_filter before vk_nlm_load");
    return VK_OK;
}

// the elapsed time between two recorded events of the handle (waits for the second)
int nlm_elapsed(vk_nlm *h, int k, double *ms) {
    *ms = 0.0;
    if (!h->timed[k]) return VK_OK;
    HIP_TRY(hipEventSynchronize(h->ev[2 * k + 1]));
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, h->ev[2 * k], h->ev[2 * k + 1]));
    *ms = (double)e;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_nlm_default_params(vk_nlm_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->search_radius = 7u; out->patch_radius = 3u; out->k = 0.45f; out->alpha = 1.0f; out->albedo_floor = 1e-3f;
    return VK_OK;
}

int vk_nlm_create(vk_scene *scene, uint32_t width, uint32_t height, vk_nlm **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if ((uint64_t)width * height > (1ull << 31) / 3 || width > 65535u || height > 65535u) return fail(VK_ERR_BAD_ARG, "image too large");
    return guarded([&]() -> int {
        std::unique_ptr<vk_nlm, void (*)(vk_nlm *)> h(new vk_nlm(), nlm_free);
        h->scene = scene; h->width = width; h->height = height;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, h->raw, nlm_pixels(h.get()) * 9u * sizeof(float));
        handle_alloc(r, h->planes, nlm_pixels(h.get()) * 12u * sizeof(float));
        if (r != VK_OK) return r;
        for (Event &e : h->ev) if ((r = e.create()) != VK_OK) return r;
        *out = h.release();
        return VK_OK;
    });
}

int vk_nlm_load(vk_nlm *h, const float *color, const float *stderr3, const float *albedo) {
    if (!h || !color || !stderr3) return fail(VK_ERR_BAD_ARG, "null argument (nlm handle, color or stderr3)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        // (color, stderr3 and, where given, albedo side by side in the handle's copy: the layout enqueue_nlm_prepare reads)
        float *const host[3] = {const_cast<float *>(color), const_cast<float *>(stderr3), const_cast<float *>(albedo)};
        const uint32_t comps[3] = {3u, 3u, 3u};
        StagedImages im;
        int rc = im.upload(h->raw, host, comps, 3, nlm_pixels(h), 0x7u);
        if (rc != VK_OK) return rc;
        h->has_albedo = albedo != nullptr;
        rc = enqueue_nlm_prepare(h, h->floor_used);
        if (rc != VK_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        h->loaded = true; h->loads++; h->last_launches = 1u;
        return VK_OK;
    });
}

int vk_nlm_load_device(vk_nlm *h, const void *d_color, const void *d_stderr3, const void *d_albedo) {
    if (!h || !d_color || !d_stderr3) return fail(VK_ERR_BAD_ARG, "null argument (nlm handle, d_color or d_stderr3)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        const size_t bytes = nlm_pixels(h) * 3u * sizeof(float);
        const void *src[3] = {d_color, d_stderr3, d_albedo};
        for (int k = 0; k < 3; k++)
            if (src[k]) HIP_TRY(hipMemcpyAsync(h->raw.get() + (size_t)k * 3u * nlm_pixels(h), src[k], bytes, hipMemcpyDeviceToDevice, nullptr));
        h->has_albedo = d_albedo != nullptr;
        int rc = enqueue_nlm_prepare(h, h->floor_used);
        if (rc != VK_OK) return rc;
        h->loaded = true; h->loads++; h->last_launches = 1u;
        return VK_OK;
    });
}

int vk_nlm_filter(vk_nlm *h, const vk_nlm_params *p, float *rgb_out, float *stderr3_out) {
    int rc = check_nlm_filter(h, p, rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        const size_t n = nlm_pixels(h), bytes = n * 3u * sizeof(float);
        if (!h->out) {
            int r = VK_OK;
            handle_alloc(r, h->out, 2u * bytes);
            if (r != VK_OK) return r;
        }
        int r = enqueue_nlm_filter(h, *p, h->out, stderr3_out ? h->out.get() + 3u * n : nullptr);
        if (r != VK_OK) return r;
        HIP_TRY(hipMemcpy(rgb_out, h->out, bytes, hipMemcpyDeviceToHost));                           // (waits for the null stream)
        if (stderr3_out) HIP_TRY(hipMemcpy(stderr3_out, h->out.get() + 3u * n, bytes, hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

int vk_nlm_filter_device(vk_nlm *h, const vk_nlm_params *p, void *d_rgb_out, void *d_stderr3_out) {
    int rc = check_nlm_filter(h, p, d_rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        return enqueue_nlm_filter(h, *p, static_cast<float *>(d_rgb_out), static_cast<float *>(d_stderr3_out));
    });
}

int vk_nlm_reset(vk_nlm *h) {
    if (!h) return fail(VK_ERR_BAD_ARG, "null nlm handle");
    h->loaded = false; h->has_albedo = false;
    return VK_OK;
}

int vk_nlm_get_info(vk_nlm *h, vk_nlm_info *out) {
    if (!h || !out) return fail(VK_ERR_BAD_ARG, "null argument (nlm handle or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        double ms = 0.0;
        int rc = nlm_elapsed(h, 1, &ms);
        if (rc != VK_OK) return rc;
        memset(out, 0, sizeof(*out));
        out->width = h->width; out->height = h->height; out->loaded = h->loaded ? 1u : 0u; out->has_albedo = h->has_albedo ? 1u : 0u;
        out->loads = h->loads; out->filters = h->filters; out->last_launches = h->last_launches; out->last_form = h->last_form;
        out->last_kernel_ms = ms;
        out->scratch_bytes = h->raw.bytes() + h->planes.bytes() + h->out.bytes();
        return VK_OK;
    });
}

void vk_nlm_destroy(vk_nlm *h) {
    if (h) nlm_free(h);
}

// test hook (vecchio_amd_debug.h): the filter kernel's form
int vk_debug_nlm_set_form(vk_nlm *h, uint32_t form) {
    if (!h) return fail(VK_ERR_BAD_ARG, "null nlm handle");
    if (form > (uint32_t)VK_NLM_FORM_TILED) return fail(VK_ERR_BAD_ARG, "unknown nlm form");
    h->form = form;
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the last prepare and filter kernels, from the events recorded around each; 0 for one not yet run
int vk_debug_nlm_last_ms(vk_nlm *h, double ms[2]) {
    if (!h || !ms) return fail(VK_ERR_BAD_ARG, "null argument (nlm handle or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(h->scene)->device));
        double got[2] = {0.0, 0.0};
        for (int k = 0; k < 2; k++) {
            int rc = nlm_elapsed(h, k, &got[k]);
            if (rc != VK_OK) return rc;
        }
        for (int k = 0; k < 2; k++) ms[k] = got[k];
        return VK_OK;
    });
}

}  // extern "C"

// ---- glare (vk_glare_*): the bright part's pyramid B_1 .. B_{L-1}, the weighted sums A_{L-2} .. A_1 on their way up and the composite
// (vk_glare.hip) on the scene's device (devices[0] of a multi-device scene); all on the null stream, on buffers and events the handle
// owns.  Nothing of the scene handle is read but its device.
struct vk_glare {
    vk_scene *scene = nullptr;                      // as handed to vk_glare_create
    uint32_t width = 0, height = 0;
    GlareDims dims;
    size_t at[GLARE_MAX_LEVELS] = {};               // where level l's plane begins in one half of `pyramid`, in floats (l >= 1)
    size_t half = 0;                                // the floats of B_1 .. B_7; A_1 .. A_7 follow them
    DeviceBuffer<float> pyramid;
    DeviceBuffer<float> io;                         // a frame in and a frame out of the host-pointer call (first vk_glare_apply)
    Event ev[2];                                    // around the last apply's kernels
    bool timed = false;
    uint32_t form = GLARE_FORM_AUTO, last_form = 0u, last_launches = 0u, last_levels = 0u;
    uint64_t applies = 0;
};

namespace {

void glare_free(vk_glare *g) {
    (void)hipSetDevice(first_part(g->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (an apply may still run)
    (void)hipGetLastError();
    delete g;
}

size_t glare_pixels(const vk_glare *g) { return (size_t)g->width * g->height; }

// Per frame size and L the form that was measured faster on the MI355X (tools/glare_report.py, DESIGN.md "Glare"): at 1920 x 1080, 900 x
// 900 and 800 x 800 with L = 4, 6 and 8 the fused form took 1.04 to 1.29 times the plain form's time per call in a stream of calls, in
// every one of the nine cells: its fewer launches do not pay for the two-level kernel's occupancy and the tail's three workgroups.  So AUTO is the plain form everywhere, and FUSED stays a debug form.
uint32_t glare_auto_form(uint32_t width, uint32_t height, uint32_t L) {
    (void)width; (void)height; (void)L;
    return GLARE_FORM_PLAIN;
}

const char *glare_refusal(const vk_glare_params &p) {
    if (p.levels < 1u || p.levels > GLARE_MAX_LEVELS) return "levels must be in 1..8";
    if (!std::isfinite(p.strength) || !(p.strength >= 0.0f) || !(p.strength <= 1.0f)) return "strength must be in [0, 1]";
    if (!std::isfinite(p.falloff) || !(p.falloff > 0.0f)) return "falloff must be finite and > 0";
    if (!std::isfinite(p.threshold) || !(p.threshold >= 0.0f)) return "threshold must be finite and >= 0";
    if (p.flags != 0u || p._pad != 0u) return "unknown glare flags";
    return nullptr;
}

int check_glare_apply(vk_glare *g, const vk_glare_params *p, const void *in, const void *out) {
    if (!g || !p || !in || !out) return fail(VK_ERR_BAD_ARG, "null argument (glare handle, params, input or output)");
    if (const char *why = glare_refusal(*p)) return fail(VK_ERR_BAD_ARG, why);
    return VK_OK;
}

// one apply from d_in into d_out (may be the same), on the handle's device; the arguments have been checked
int enqueue_glare(vk_glare *g, const vk_glare_params &p, const float *d_in, float *d_out) {
    const uint32_t L = p.levels;
    const uint32_t form = g->form == GLARE_FORM_AUTO ? glare_auto_form(g->width, g->height, L) : g->form;
    const GlareDims &d = g->dims;
    float c[GLARE_MAX_LEVELS];
    glare_weights(L, p.falloff, c);
    auto B = [&](uint32_t l) { return g->pyramid.get() + g->at[l]; };
    auto A = [&](uint32_t l) { return g->pyramid.get() + g->half + g->at[l]; };
    uint32_t launches = 0u;
    HIP_TRY(hipEventRecord(g->ev[0], nullptr));
    // the level the up passes start from, and whether it is a stored A (the tail's) or c_{L-1} * B_{L-1}
    uint32_t top = L - 1u;
    bool top_is_a = false;
    if (form == GLARE_FORM_PLAIN) {
        for (uint32_t l = 0; l + 1u < L; l++) {
            GlareDownArgs D;
            memset(&D, 0, sizeof(D));
            D.src = l ? B(l) : d_in; D.dst = B(l + 1u); D.sw = (uint32_t)d.w[l]; D.sh = (uint32_t)d.h[l]; D.threshold = p.threshold;
            launch_glare_down(D, l == 0u, false);
            launches++;
        }
    } else {
        const uint32_t t = glare_tail_level(d);
        const bool tail = t + 2u <= L;
        const uint32_t m = tail ? t : L - 1u;
        uint32_t l = 0u;
        if (m >= 2u) {
            GlareDown2Args D;
            memset(&D, 0, sizeof(D));
            D.src = d_in; D.b1 = B(1u); D.b2 = B(2u); D.sw = g->width; D.sh = g->height; D.threshold = p.threshold;
            launch_glare_down2(D);
            launches++;
            l = 2u;
        }
        for (; l < m; l++) {
            GlareDownArgs D;
            memset(&D, 0, sizeof(D));
            D.src = l ? B(l) : d_in; D.dst = B(l + 1u); D.sw = (uint32_t)d.w[l]; D.sh = (uint32_t)d.h[l]; D.threshold = p.threshold;
            launch_glare_down(D, l == 0u, true);
            launches++;
        }
        if (tail) {
            GlareTailArgs T;
            memset(&T, 0, sizeof(T));
            T.bt = B(t); T.at = A(t); T.w = (uint32_t)d.w[t]; T.h = (uint32_t)d.h[t]; T.t = t; T.levels = L;
            for (uint32_t k = 0; k < GLARE_MAX_LEVELS; k++) T.c[k] = c[k];
            launch_glare_tail(T);
            launches++;
            top = t; top_is_a = true;
        }
    }
    HIP_TRY(hipGetLastError());
    for (uint32_t l = top; l-- > 1u;) {
        GlareUpArgs U;
        memset(&U, 0, sizeof(U));
        U.src = top_is_a || l + 1u < top ? A(l + 1u) : B(l + 1u); U.scale = top_is_a || l + 1u < top ? 1.0f : c[top];
        U.b = B(l); U.dst = A(l); U.w = (uint32_t)d.w[l]; U.h = (uint32_t)d.h[l]; U.c = c[l];
        launch_glare_up(U);
        launches++;
    }
    GlareCompositeArgs C;
    memset(&C, 0, sizeof(C));
    C.in = d_in; C.out = d_out; C.w = g->width; C.h = g->height; C.c0 = c[0]; C.strength = p.strength; C.threshold = p.threshold;
    C.scale = 1.0f;
    if (L >= 2u) {
        const bool stored = top_is_a || top > 1u;
        C.src = stored ? A(1u) : B(1u); C.scale = stored ? 1.0f : c[1];
    }
    launch_glare_composite(C);
    launches++;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->ev[1], nullptr));
    g->timed = true;
    g->last_form = form; g->last_launches = launches; g->last_levels = L; g->applies++;
    return VK_OK;
}

int glare_elapsed(vk_glare *g, double *ms) {
    *ms = 0.0;
    if (!g->timed) return VK_OK;
    HIP_TRY(hipEventSynchronize(g->ev[1]));
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, g->ev[0], g->ev[1]));
    *ms = (double)e;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_glare_default_params(vk_glare_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->levels = 6u; out->strength = 0.15f; out->falloff = 1.0f; out->threshold = 0.0f;
    return VK_OK;
}

int vk_glare_create(vk_scene *scene, uint32_t width, uint32_t height, vk_glare **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if ((uint64_t)width * height > (1ull << 31) / 3 || width > 65535u || height > 65535u) return fail(VK_ERR_BAD_ARG, "image too large");
    return guarded([&]() -> int {
        std::unique_ptr<vk_glare, void (*)(vk_glare *)> g(new vk_glare(), glare_free);
        g->scene = scene; g->width = width; g->height = height;
        g->dims = glare_dims(width, height);
        for (uint32_t l = 1; l < GLARE_MAX_LEVELS; l++) {
            g->at[l] = g->half;
            g->half += (size_t)g->dims.w[l] * (size_t)g->dims.h[l] * 3u;
        }
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, g->pyramid, 2u * g->half * sizeof(float));
        if (r != VK_OK) return r;
        for (Event &e : g->ev) if ((r = e.create()) != VK_OK) return r;
        *out = g.release();
        return VK_OK;
    });
}

int vk_glare_apply(vk_glare *g, const vk_glare_params *p, const float *rgb_in, float *rgb_out) {
    int rc = check_glare_apply(g, p, rgb_in, rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        // (the frame in and the frame out side by side in the handle's buffer; only the first is uploaded, only the second comes back)
        float *const host[2] = {const_cast<float *>(rgb_in), rgb_out};
        const uint32_t comps[2] = {3u, 3u};
        StagedImages im;
        int r = im.upload(g->io, host, comps, 2, glare_pixels(g), 0x1u);
        if (r != VK_OK) return r;
        r = enqueue_glare(g, *p, im.dev[0], im.dev[1]);
        if (r != VK_OK) return r;
        return im.download(0x2u);                                                         // (waits for the null stream)
    });
}

int vk_glare_apply_device(vk_glare *g, const vk_glare_params *p, const void *d_rgb_in, void *d_rgb_out) {
    int rc = check_glare_apply(g, p, d_rgb_in, d_rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        return enqueue_glare(g, *p, static_cast<const float *>(d_rgb_in), static_cast<float *>(d_rgb_out));
    });
}

int vk_glare_get_info(vk_glare *g, vk_glare_info *out) {
    if (!g || !out) return fail(VK_ERR_BAD_ARG, "null argument (glare handle or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        double ms = 0.0;
        int rc = glare_elapsed(g, &ms);
        if (rc != VK_OK) return rc;
        memset(out, 0, sizeof(*out));
        out->width = g->width; out->height = g->height; out->applies = g->applies;
        out->last_levels = g->last_levels; out->last_form = g->last_form; out->last_launches = g->last_launches;
        out->last_kernel_ms = ms;
        out->scratch_bytes = g->pyramid.bytes() + g->io.bytes();
        return VK_OK;
    });
}

void vk_glare_destroy(vk_glare *g) {
    if (g) glare_free(g);
}

// test hook (vecchio_amd_debug.h): the form of the apply's kernels
int vk_debug_glare_set_form(vk_glare *g, uint32_t form) {
    if (!g) return fail(VK_ERR_BAD_ARG, "null glare handle");
    if (form > (uint32_t)VK_GLARE_FORM_FUSED) return fail(VK_ERR_BAD_ARG, "unknown glare form");
    g->form = form;
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the last apply's kernels, from the events recorded around them; 0 before one
int vk_debug_glare_last_ms(vk_glare *g, double *ms) {
    if (!g || !ms) return fail(VK_ERR_BAD_ARG, "null argument (glare handle or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        double got = 0.0;
        int rc = glare_elapsed(g, &got);
        if (rc != VK_OK) return rc;
        *ms = got;
        return VK_OK;
    });
}

}  // extern "C"

// ---- point-spread function (vk_psf_*): the three planes F of a frame's transform, the three planes G of the loaded kernel's, the
// twiddle tables of the two padded sizes and the transform kernels (vk_psf.hip) on the scene's device (devices[0] of a multi-device
// scene); all on the null stream, on buffers and events the handle owns.  Nothing of the scene handle is read but its device.
struct vk_psf {
    vk_scene *scene = nullptr;                      // as handed to vk_psf_create
    uint32_t width = 0, height = 0, kmax = 0;
    uint32_t K = 0, Px = 0, Py = 0;                 // of the loaded kernel; K = 0: none
    DeviceBuffer<PsfC> F, G;                        // three planes each, sized for kmax
    DeviceBuffer<PsfC> tw;                          // T of Px, then T of Py
    DeviceBuffer<float> kern;                       // the normalised kernel
    DeviceBuffer<float> keep;                       // the input of an in-place apply in the LDS form (first such apply)
    DeviceBuffer<float> io;                         // a frame in and a frame out of the host-pointer call (first vk_psf_apply)
    Event ev[2];                                    // around the last apply's kernels
    Event pass_ev[3];                               // between the four passes of an apply in the LDS form
    bool timed = false;
    uint32_t last_form = 0u, last_launches = 0u;
    uint64_t loads = 0, applies = 0;
};

namespace {

void psf_free(vk_psf *g) {
    (void)hipSetDevice(first_part(g->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (an apply may still run)
    (void)hipGetLastError();
    delete g;
}

size_t psf_pixels(const vk_psf *g) { return (size_t)g->width * g->height; }

// AUTO is the LDS form everywhere: four launches that move each plane once per pass, against PLAIN's launch per butterfly stage, each of
// which reads and writes every plane (48 launches at 2048 x 2048).  tools/psf_report.py times both; its table is not recorded yet
// (DESIGN.md "Point-spread function"), so this rule rests on that count and is the thing to revisit when it is.
uint32_t psf_auto_form(uint32_t width, uint32_t height, uint32_t K) {
    (void)width; (void)height; (void)K;
    return PSF_FORM_LDS;
}

const char *psf_refusal(const vk_psf_params &p) {
    if (!std::isfinite(p.strength) || !(p.strength >= 0.0f) || !(p.strength <= 1.0f)) return "strength must be in [0, 1]";
    if (!std::isfinite(p.threshold) || !(p.threshold >= 0.0f)) return "threshold must be finite and >= 0";
    if (p.form > PSF_FORM_LDS) return "unknown psf form";
    if (p.flags != 0u || p._pad != 0u) return "unknown psf flags";
    return nullptr;
}

int check_psf_apply(vk_psf *g, const vk_psf_params *p, const void *in, const void *out) {
    if (!g || !p || !in || !out) return fail(VK_ERR_BAD_ARG, "null argument (psf handle, params, input or output)");
    if (const char *why = psf_refusal(*p)) return fail(VK_ERR_BAD_ARG, why);
    if (g->K == 0u) return fail(VK_ERR_BAD_ARG, "vk_psf_apply before vk_psf_load");
    return VK_OK;
}

int check_psf_load(vk_psf *g, uint32_t K, const void *kernel) {
    if (!g || !kernel) return fail(VK_ERR_BAD_ARG, "null argument (psf handle or kernel)");
    if (K < PSF_MIN_K || K > PSF_MAX_K || (K & 1u) == 0u) return fail(VK_ERR_BAD_ARG, "K must be odd and in 3..1023");
    if (K > g->kmax) return fail(VK_ERR_BAD_ARG, "K exceeds the handle's kmax");
    return VK_OK;
}

// one bare 2-D transform of `planes` planes in place, rows then columns, in the given form (PLAIN or LDS); *launches counts its kernels
void enqueue_psf_fft2(PsfC *a, uint32_t planes, uint32_t Px, uint32_t Py, const PsfC *Tx, const PsfC *Ty, bool inverse, bool scaled,
    uint32_t form, uint32_t *launches) {
    const float scale = 1.0f / ((float)Px * (float)Py);
    if (form == PSF_FORM_PLAIN) {
        for (uint32_t axis = 0; axis < 2u; axis++) {
            PsfStageArgs S;
            memset(&S, 0, sizeof(S));
            S.a = a; S.T = axis ? Ty : Tx; S.Px = Px; S.Py = Py; S.planes = planes; S.axis = axis; S.inverse = inverse ? 1u : 0u;
            launch_psf_bitrev(S);
            ++*launches;
            const uint32_t m = psf_log2(axis ? Py : Px);
            for (S.s = 1u; S.s <= m; S.s++) { launch_psf_stage(S); ++*launches; }
        }
        if (inverse && scaled) {
            PsfScaleArgs C;
            memset(&C, 0, sizeof(C));
            C.a = a; C.n = (uint64_t)planes * Px * Py; C.scale = scale;
            launch_psf_scale(C);
            ++*launches;
        }
        return;
    }
    for (uint32_t axis = 0; axis < 2u; axis++) {
        PsfLineArgs A;
        memset(&A, 0, sizeof(A));
        A.a = a; A.T = axis ? Ty : Tx; A.Px = Px; A.Py = Py; A.planes = planes; A.count = axis ? Px : Py;
        A.lines = psf_line_tile(axis ? Py : Px, axis != 0u, A.count);
        A.load = PSF_LOAD_PLANE; A.store = axis && inverse && scaled ? PSF_STORE_SCALED : PSF_STORE_PLANE;
        A.inverse = inverse ? 1u : 0u; A.scale = scale;
        launch_psf_line(A, axis != 0u);
        ++*launches;
    }
}

// the kernel in g->kern (normalised, K x K x 3) into G: placed, then transformed
int enqueue_psf_kernel(vk_psf *g, uint32_t K) {
    const uint32_t Px = psf_pow2(g->width + K - 1u), Py = psf_pow2(g->height + K - 1u);
    const std::vector<PsfC> Tx = psf_twiddles(Px), Ty = psf_twiddles(Py);
    HIP_TRY(hipMemcpy(g->tw.get(), Tx.data(), Tx.size() * sizeof(PsfC), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->tw.get() + Px / 2u, Ty.data(), Ty.size() * sizeof(PsfC), hipMemcpyHostToDevice));
    PsfPlaceArgs P;
    memset(&P, 0, sizeof(P));
    P.kernel = g->kern; P.G = g->G; P.K = K; P.Px = Px; P.Py = Py;
    launch_psf_place(P);
    uint32_t launches = 1u;
    enqueue_psf_fft2(g->G, 3u, Px, Py, g->tw.get(), g->tw.get() + Px / 2u, false, false, psf_auto_form(g->width, g->height, K), &launches);
    HIP_TRY(hipGetLastError());
    g->K = K; g->Px = Px; g->Py = Py; g->loads++; g->last_launches = launches;
    return VK_OK;
}

// validates and normalises the caller's kernel (host memory) and makes G of it
int psf_load_host(vk_psf *g, uint32_t K, const float *kernel) {
    std::vector<float> norm((size_t)K * K * 3u);
    if (const char *why = psf_normalise(K, kernel, norm.data())) return fail(VK_ERR_BAD_ARG, why);
    HIP_TRY(hipStreamSynchronize(nullptr));              // (an apply may still read the planes and tables this replaces)
    HIP_TRY(hipMemcpy(g->kern.get(), norm.data(), norm.size() * sizeof(float), hipMemcpyHostToDevice));
    return enqueue_psf_kernel(g, K);
}

// one apply from d_in into d_out (may be the same), on the handle's device; the arguments have been checked
int enqueue_psf(vk_psf *g, const vk_psf_params &p, const float *d_in, float *d_out) {
    const uint32_t form = p.form == PSF_FORM_AUTO ? psf_auto_form(g->width, g->height, g->K) : p.form;
    const uint32_t W = g->width, H = g->height, Px = g->Px, Py = g->Py;
    const PsfC *Tx = g->tw.get(), *Ty = g->tw.get() + Px / 2u;
    const float scale = 1.0f / ((float)Px * (float)Py);
    uint32_t launches = 0u;
    if (form == PSF_FORM_LDS && d_in == d_out) {
        // (the last pass writes a component of a pixel while the workgroups of the other components read the pixel: from a copy, then)
        int rc = g->keep.ensure(psf_pixels(g) * 3u * sizeof(float));
        if (rc != VK_OK) return rc;
        HIP_TRY(hipMemcpyAsync(g->keep.get(), d_in, psf_pixels(g) * 3u * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        d_in = g->keep.get();
    }
    HIP_TRY(hipEventRecord(g->ev[0], nullptr));
    if (form == PSF_FORM_PLAIN) {
        PsfPadArgs P;
        memset(&P, 0, sizeof(P));
        P.in = d_in; P.F = g->F; P.W = W; P.H = H; P.Px = Px; P.Py = Py; P.threshold = p.threshold;
        launch_psf_pad(P);
        launches++;
        enqueue_psf_fft2(g->F, 3u, Px, Py, Tx, Ty, false, false, PSF_FORM_PLAIN, &launches);
        PsfProductArgs M;
        memset(&M, 0, sizeof(M));
        M.F = g->F; M.G = g->G; M.n = (uint64_t)3u * Px * Py;
        launch_psf_product(M);
        launches++;
        enqueue_psf_fft2(g->F, 3u, Px, Py, Tx, Ty, true, false, PSF_FORM_PLAIN, &launches);
        PsfCompositeArgs C;
        memset(&C, 0, sizeof(C));
        C.in = d_in; C.out = d_out; C.F = g->F; C.W = W; C.H = H; C.Px = Px; C.Py = Py;
        C.scale = scale; C.strength = p.strength; C.threshold = p.threshold;
        launch_psf_composite(C);
        launches++;
    } else {
        PsfLineArgs A;
        memset(&A, 0, sizeof(A));
        A.a = g->F; A.G = g->G; A.in = d_in; A.out = d_out; A.Px = Px; A.Py = Py; A.planes = 3u; A.W = W; A.H = H; A.valid = H;
        A.scale = scale; A.strength = p.strength; A.threshold = p.threshold;
        // rows forward, from the frame: rows >= H are all zero and are neither made nor read
        A.T = Tx; A.count = H; A.lines = psf_line_tile(Px, false, A.count); A.load = PSF_LOAD_FRAME; A.store = PSF_STORE_PLANE;
        launch_psf_line(A, false);
        HIP_TRY(hipEventRecord(g->pass_ev[0], nullptr));
        // columns forward
        A.T = Ty; A.count = Px; A.lines = psf_line_tile(Py, true, A.count); A.load = PSF_LOAD_ROWS;
        launch_psf_line(A, true);
        HIP_TRY(hipEventRecord(g->pass_ev[1], nullptr));
        // rows inverse, of the product
        A.inverse = 1u;
        A.T = Tx; A.count = Py; A.lines = psf_line_tile(Px, false, A.count); A.load = PSF_LOAD_PRODUCT;
        launch_psf_line(A, false);
        HIP_TRY(hipEventRecord(g->pass_ev[2], nullptr));
        // columns inverse, into the frame: only the columns the frame has
        A.T = Ty; A.count = W; A.lines = psf_line_tile(Py, true, A.count); A.load = PSF_LOAD_PLANE; A.store = PSF_STORE_FRAME;
        launch_psf_line(A, true);
        launches = 4u;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->ev[1], nullptr));
    g->timed = true;
    g->last_form = form; g->last_launches = launches; g->applies++;
    return VK_OK;
}

int psf_elapsed(vk_psf *g, double *ms) {
    *ms = 0.0;
    if (!g->timed) return VK_OK;
    HIP_TRY(hipEventSynchronize(g->ev[1]));
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, g->ev[0], g->ev[1]));
    *ms = (double)e;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_psf_default_params(vk_psf_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->strength = 0.15f; out->threshold = 0.0f; out->form = PSF_FORM_AUTO;
    return VK_OK;
}

int vk_psf_star(uint32_t K, uint32_t streaks, float rotation, float sharpness, float chroma, float *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (K < PSF_MIN_K || K > PSF_MAX_K || (K & 1u) == 0u) return fail(VK_ERR_BAD_ARG, "K must be odd and in 3..1023");
    if (streaks > 64u) return fail(VK_ERR_BAD_ARG, "streaks must be in 0..64");
    if (!std::isfinite(rotation)) return fail(VK_ERR_BAD_ARG, "rotation must be finite");
    if (!std::isfinite(sharpness) || !(sharpness >= 1.0f)) return fail(VK_ERR_BAD_ARG, "sharpness must be finite and >= 1");
    if (!std::isfinite(chroma) || !(chroma >= 0.0f) || !(chroma <= 0.5f)) return fail(VK_ERR_BAD_ARG, "chroma must be in [0, 0.5]");
    psf_star(K, streaks, rotation, sharpness, chroma, out);
    return VK_OK;
}

int vk_psf_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t kmax, vk_psf **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (width == 0u || height == 0u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if (kmax < PSF_MIN_K || kmax > PSF_MAX_K || (kmax & 1u) == 0u) return fail(VK_ERR_BAD_ARG, "kmax must be odd and in 3..1023");
    if ((uint64_t)width + kmax - 1u > PSF_MAX_N || (uint64_t)height + kmax - 1u > PSF_MAX_N)
        return fail(VK_ERR_BAD_ARG, "padded size exceeds 4096");
    return guarded([&]() -> int {
        std::unique_ptr<vk_psf, void (*)(vk_psf *)> g(new vk_psf(), psf_free);
        g->scene = scene; g->width = width; g->height = height; g->kmax = kmax;
        const size_t Px = psf_pow2(width + kmax - 1u), Py = psf_pow2(height + kmax - 1u);
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, g->F, 3u * Px * Py * sizeof(PsfC));
        handle_alloc(r, g->G, 3u * Px * Py * sizeof(PsfC));
        handle_alloc(r, g->tw, (Px / 2u + Py / 2u) * sizeof(PsfC));
        handle_alloc(r, g->kern, (size_t)kmax * kmax * 3u * sizeof(float));
        if (r != VK_OK) return r;
        for (Event &e : g->ev) if ((r = e.create()) != VK_OK) return r;
        for (Event &e : g->pass_ev) if ((r = e.create()) != VK_OK) return r;
        *out = g.release();
        return VK_OK;
    });
}

int vk_psf_load(vk_psf *g, uint32_t K, const float *kernel) {
    int rc = check_psf_load(g, K, kernel);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        int r = psf_load_host(g, K, kernel);
        if (r != VK_OK) return r;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return VK_OK;
    });
}

int vk_psf_load_device(vk_psf *g, uint32_t K, const void *d_kernel) {
    int rc = check_psf_load(g, K, d_kernel);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        // (the kernel is checked and normalised in f64 on the host: it comes back first, which waits for the null stream)
        std::vector<float> host((size_t)K * K * 3u);
        HIP_TRY(hipMemcpy(host.data(), d_kernel, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        return psf_load_host(g, K, host.data());
    });
}

int vk_psf_apply(vk_psf *g, const vk_psf_params *p, const float *rgb_in, float *rgb_out) {
    int rc = check_psf_apply(g, p, rgb_in, rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        // (the frame in and the frame out side by side in the handle's buffer; only the first is uploaded, only the second comes back)
        float *const host[2] = {const_cast<float *>(rgb_in), rgb_out};
        const uint32_t comps[2] = {3u, 3u};
        StagedImages im;
        int r = im.upload(g->io, host, comps, 2, psf_pixels(g), 0x1u);
        if (r != VK_OK) return r;
        r = enqueue_psf(g, *p, im.dev[0], im.dev[1]);
        if (r != VK_OK) return r;
        return im.download(0x2u);                                                         // (waits for the null stream)
    });
}

int vk_psf_apply_device(vk_psf *g, const vk_psf_params *p, const void *d_rgb_in, void *d_rgb_out) {
    int rc = check_psf_apply(g, p, d_rgb_in, d_rgb_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        return enqueue_psf(g, *p, static_cast<const float *>(d_rgb_in), static_cast<float *>(d_rgb_out));
    });
}

int vk_psf_reset(vk_psf *g) {
    if (!g) return fail(VK_ERR_BAD_ARG, "null psf handle");
    g->K = 0u; g->Px = 0u; g->Py = 0u;
    return VK_OK;
}

int vk_psf_get_info(vk_psf *g, vk_psf_info *out) {
    if (!g || !out) return fail(VK_ERR_BAD_ARG, "null argument (psf handle or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        double ms = 0.0;
        int rc = psf_elapsed(g, &ms);
        if (rc != VK_OK) return rc;
        memset(out, 0, sizeof(*out));
        out->width = g->width; out->height = g->height; out->K = g->K; out->Px = g->Px; out->Py = g->Py; out->kmax = g->kmax;
        out->loads = g->loads; out->applies = g->applies; out->last_form = g->last_form; out->last_launches = g->last_launches;
        out->last_kernel_ms = ms;
        out->scratch_bytes = g->F.bytes() + g->G.bytes() + g->tw.bytes() + g->kern.bytes() + g->keep.bytes() + g->io.bytes();
        return VK_OK;
    });
}

void vk_psf_destroy(vk_psf *g) {
    if (g) psf_free(g);
}

// test hook (vecchio_amd_debug.h): the four passes of the last apply, from the events recorded between them; zeros unless it was in the
// LDS form
int vk_psf_debug_last_pass_ms(vk_psf *g, double ms[4]) {
    if (!g || !ms) return fail(VK_ERR_BAD_ARG, "null argument (psf handle or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(g->scene)->device));
        double got[4] = {0.0, 0.0, 0.0, 0.0};
        if (g->timed && g->last_form == PSF_FORM_LDS) {
            HIP_TRY(hipEventSynchronize(g->ev[1]));
            const hipEvent_t at[5] = {g->ev[0], g->pass_ev[0], g->pass_ev[1], g->pass_ev[2], g->ev[1]};
            for (int k = 0; k < 4; k++) {
                float e = 0.0f;
                HIP_TRY(hipEventElapsedTime(&e, at[k], at[k + 1]));
                got[k] = (double)e;
            }
        }
        for (int k = 0; k < 4; k++) ms[k] = got[k];
        return VK_OK;
    });
}

// test hook (vecchio_amd_debug.h): the library's twiddle table of a length N: N / 2 entries, (re, im) pairs.  Touches no device.
int vk_psf_debug_twiddles(uint32_t N, float *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (N < 2u || N > PSF_MAX_N || (N & (N - 1u)) != 0u) return fail(VK_ERR_BAD_ARG, "N must be a power of two in 2..4096");
    const std::vector<PsfC> T = psf_twiddles(N);
    memcpy(out, T.data(), T.size() * sizeof(PsfC));
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): one bare 2-D transform of the caller's Px x Py complex values (host memory), in place
int vk_psf_debug_fft2(vk_scene *scene, uint32_t Px, uint32_t Py, uint32_t inverse, uint32_t form, float *data) {
    if (!scene || !data) return fail(VK_ERR_BAD_ARG, "null argument (scene or data)");
    for (uint32_t N : {Px, Py})
        if (N < 2u || N > PSF_MAX_N || (N & (N - 1u)) != 0u) return fail(VK_ERR_BAD_ARG, "Px and Py must be powers of two in 2..4096");
    if (inverse > 1u) return fail(VK_ERR_BAD_ARG, "inverse must be 0 or 1");
    if (form != PSF_FORM_PLAIN && form != PSF_FORM_LDS) return fail(VK_ERR_BAD_ARG, "unknown psf form");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        const size_t n = (size_t)Px * Py;
        DeviceBuffer<PsfC> a, tw;
        int r = VK_OK;
        handle_alloc(r, a, n * sizeof(PsfC));
        handle_alloc(r, tw, (Px / 2u + Py / 2u) * sizeof(PsfC));
        if (r != VK_OK) return r;
        const std::vector<PsfC> Tx = psf_twiddles(Px), Ty = psf_twiddles(Py);
        HIP_TRY(hipMemcpy(tw.get(), Tx.data(), Tx.size() * sizeof(PsfC), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(tw.get() + Px / 2u, Ty.data(), Ty.size() * sizeof(PsfC), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(a.get(), data, n * sizeof(PsfC), hipMemcpyHostToDevice));
        uint32_t launches = 0u;
        enqueue_psf_fft2(a, 1u, Px, Py, tw.get(), tw.get() + Px / 2u, inverse != 0u, true, form, &launches);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(data, a.get(), n * sizeof(PsfC), hipMemcpyDeviceToHost));      // (waits for the null stream)
        return VK_OK;
    });
}

}  // extern "C"

// ---- guided upsampling (vk_upsample_*): a copy of the loaded low images on the scene's device (devices[0] of a multi-device scene), the
// three planes upsample_prepare_kernel makes of it and the filter over the high frame (vk_upsample.hip); all on the null stream, on
// buffers and events the handle owns.  Nothing of the scene handle is read but its device.
struct vk_upsample {
    vk_scene *scene = nullptr;                      // as handed to vk_upsample_create
    uint32_t w = 0, h = 0, W = 0, H = 0;
    DeviceBuffer<float> raw;                        // color, stderr3, albedo, normal, depth as loaded: room for 13 floats a low pixel
    float *raw_at[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // where each loaded image is in `raw`; null = not loaded
    DeviceBuffer<UpRec> planes;                     // P0, P1, P2: [3][w * h]
    DeviceBuffer<uint32_t> counts;                  // fallback_pixels, empty_pixels of the last apply
    DeviceBuffer<float> io;                         // the high guides in and the two frames out of the host-pointer call (first vk_upsample_apply)
    Event ev[2];                                    // around the last apply's filter kernel
    bool timed = false, loaded = false;
    float floor_used = 1e-3f;                       // the albedo_floor the planes were prepared with
    uint32_t form = UPSAMPLE_FORM_AUTO, last_form = 0u, last_launches = 0u;
    uint64_t loads = 0, applies = 0;
};

namespace {

void upsample_free(vk_upsample *u) {
    (void)hipSetDevice(first_part(u->scene)->device);
    (void)hipStreamSynchronize(nullptr);              // (an apply or a copy may still run)
    (void)hipGetLastError();
    delete u;
}

size_t upsample_lo(const vk_upsample *u) { return (size_t)u->w * u->h; }
size_t upsample_hi(const vk_upsample *u) { return (size_t)u->W * u->H; }

uint32_t upsample_guides(const vk_upsample *u) {
    return (u->raw_at[1] ? (uint32_t)VK_UPSAMPLE_HAS_STDERR : 0u) | (u->raw_at[2] ? (uint32_t)VK_UPSAMPLE_HAS_ALBEDO : 0u) |
        (u->raw_at[3] ? (uint32_t)VK_UPSAMPLE_HAS_NORMAL : 0u) | (u->raw_at[4] ? (uint32_t)VK_UPSAMPLE_HAS_DEPTH : 0u);
}

const char *upsample_refusal(const vk_upsample_params &p) {
    if (!std::isfinite(p.sigma_z) || !(p.sigma_z > 0.0f)) return "sigma_z must be finite and > 0";
    if (p.normal_squarings > 10u) return "normal_squarings must be in 0..10";
    if (!std::isfinite(p.albedo_floor) || !(p.albedo_floor > 0.0f)) return "albedo_floor must be finite and > 0";
    if (p.flags != 0u || p._pad != 0u) return "unknown upsample flags";
    return nullptr;
}

// the prepare kernel over the handle's copy of the loaded images, into its planes
int enqueue_upsample_prepare(vk_upsample *u, float albedo_floor) {
    const size_t n = upsample_lo(u);
    UpsamplePrepareArgs A;
    memset(&A, 0, sizeof(A));
    A.color = u->raw_at[0]; A.stderr3 = u->raw_at[1]; A.albedo = u->raw_at[2]; A.normal = u->raw_at[3]; A.depth = u->raw_at[4];
    A.P0 = u->planes; A.P1 = u->planes.get() + n; A.P2 = u->planes.get() + 2u * n;
    A.w = u->w; A.h = u->h; A.albedo_floor = albedo_floor;
    launch_upsample_prepare(A);
    HIP_TRY(hipGetLastError());
    u->floor_used = albedo_floor;
    return VK_OK;
}

// one apply into d_out and d_se (may be null), on the handle's device; the arguments have been checked
int enqueue_upsample(vk_upsample *u, const vk_upsample_params &p, const float *d_albedo, const float *d_normal, const float *d_depth,
    float *d_out, float *d_se) {
    const size_t n = upsample_lo(u);
    u->last_launches = 0u;
    if (u->raw_at[2] && p.albedo_floor != u->floor_used) {
        int rc = enqueue_upsample_prepare(u, p.albedo_floor);
        if (rc != VK_OK) return rc;
        u->last_launches++;
    }
    UpsampleArgs A;
    memset(&A, 0, sizeof(A));
    A.P0 = u->planes; A.P1 = u->planes.get() + n; A.P2 = u->planes.get() + 2u * n;
    A.albedo_hi = d_albedo; A.normal_hi = d_normal; A.depth_hi = d_depth;
    A.out = d_out; A.stderr3_out = d_se; A.counts = u->counts;
    A.w = u->w; A.h = u->h; A.W = u->W; A.H = u->H;
    upsample_ratios(u->w, u->W, A.rx, A.sx);
    upsample_ratios(u->h, u->H, A.ry, A.sy);
    A.sigma_z = p.sigma_z; A.albedo_floor = p.albedo_floor; A.normal_squarings = p.normal_squarings;
    A.flags = (d_normal && u->raw_at[3] ? UP_NORMAL : 0u) | (d_depth && u->raw_at[4] ? UP_DEPTH : 0u);
    const uint32_t form = u->form == UPSAMPLE_FORM_AUTO ? upsample_auto_form(u->w, u->h, u->W, u->H) : u->form;
    HIP_TRY(hipMemsetAsync(u->counts, 0, 2u * sizeof(uint32_t), nullptr));
    HIP_TRY(hipEventRecord(u->ev[0], nullptr));
    launch_upsample_apply(A, form);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(u->ev[1], nullptr));
    u->timed = true;
    u->last_form = form; u->last_launches++; u->applies++;
    return VK_OK;
}

int check_upsample_apply(vk_upsample *u, const vk_upsample_params *p, const void *albedo, const void *out, const void *se) {
    if (!u || !p || !out) return fail(VK_ERR_BAD_ARG, "null argument (upsample handle, params or output)");
    if (const char *why = upsample_refusal(*p)) return fail(VK_ERR_BAD_ARG, why);
    if (!u->loaded) return fail(VK_ERR_BAD_ARG, "vk_upsample_apply before vk_upsample_load");
    if ((albedo != nullptr) != (u->raw_at[2] != nullptr)) return fail(VK_ERR_BAD_ARG, "albedo must be given at both sizes or at neither");
    if (se && !u->raw_at[1]) return fail(VK_ERR_BAD_ARG, "stderr3_out wanted but no stderr3 was loaded");
    return VK_OK;
}

int upsample_elapsed(vk_upsample *u, double *ms) {
    *ms = 0.0;
    if (!u->timed) return VK_OK;
    HIP_TRY(hipEventSynchronize(u->ev[1]));
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, u->ev[0], u->ev[1]));
    *ms = (double)e;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_upsample_default_params(vk_upsample_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->sigma_z = 1.0f; out->normal_squarings = 7u; out->albedo_floor = 1e-3f;
    return VK_OK;
}

int vk_upsample_create(vk_scene *scene, uint32_t w, uint32_t h, uint32_t W, uint32_t H, vk_upsample **out) {
    if (!scene || !out) return fail(VK_ERR_BAD_ARG, "null argument (scene or out)");
    if (w < 2u || h < 2u) return fail(VK_ERR_BAD_ARG, "the low width and height must be >= 2");
    if (w > W || h > H) return fail(VK_ERR_BAD_ARG, "the low size must not exceed the high size");
    if ((uint64_t)W * H > (1ull << 31) / 3 || W > 65535u || H > 65535u) return fail(VK_ERR_BAD_ARG, "image too large");
    return guarded([&]() -> int {
        std::unique_ptr<vk_upsample, void (*)(vk_upsample *)> u(new vk_upsample(), upsample_free);
        u->scene = scene; u->w = w; u->h = h; u->W = W; u->H = H;
        HIP_TRY(hipSetDevice(first_part(scene)->device));
        int r = VK_OK;
        handle_alloc(r, u->raw, upsample_lo(u.get()) * 13u * sizeof(float));
        handle_alloc(r, u->planes, upsample_lo(u.get()) * 3u * sizeof(UpRec));
        handle_alloc(r, u->counts, 2u * sizeof(uint32_t));
        if (r != VK_OK) return r;
        HIP_TRY(hipMemsetAsync(u->counts, 0, 2u * sizeof(uint32_t), nullptr));
        for (Event &e : u->ev) if ((r = e.create()) != VK_OK) return r;
        *out = u.release();
        return VK_OK;
    });
}

int vk_upsample_load(vk_upsample *u, const float *color_lo, const float *stderr3_lo, const float *albedo_lo, const float *normal_lo,
    const float *depth_lo) {
    if (!u || !color_lo) return fail(VK_ERR_BAD_ARG, "null argument (upsample handle or color_lo)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        HIP_TRY(hipStreamSynchronize(nullptr));              // (an apply may still read the planes the copies' prepare will replace)
        // (the given images side by side in the handle's copy, which has room for all five)
        float *const host[5] = {const_cast<float *>(color_lo), const_cast<float *>(stderr3_lo), const_cast<float *>(albedo_lo),
                                const_cast<float *>(normal_lo), const_cast<float *>(depth_lo)};
        const uint32_t comps[5] = {3u, 3u, 3u, 3u, 1u};
        StagedImages im;
        u->loaded = false;
        int rc = im.upload(u->raw, host, comps, 5, upsample_lo(u), 0x1Fu);
        if (rc != VK_OK) return rc;
        for (int k = 0; k < 5; k++) u->raw_at[k] = im.dev[k];
        rc = enqueue_upsample_prepare(u, u->floor_used);
        if (rc != VK_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        u->loaded = true; u->loads++; u->last_launches = 1u;
        return VK_OK;
    });
}

int vk_upsample_load_device(vk_upsample *u, const void *d_color_lo, const void *d_stderr3_lo, const void *d_albedo_lo,
    const void *d_normal_lo, const void *d_depth_lo) {
    if (!u || !d_color_lo) return fail(VK_ERR_BAD_ARG, "null argument (upsample handle or d_color_lo)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        const size_t n = upsample_lo(u);
        const void *src[5] = {d_color_lo, d_stderr3_lo, d_albedo_lo, d_normal_lo, d_depth_lo};
        u->loaded = false;
        for (int k = 0; k < 5; k++) {
            u->raw_at[k] = src[k] ? u->raw.get() + (size_t)k * 3u * n : nullptr;
            if (src[k]) HIP_TRY(hipMemcpyAsync(u->raw_at[k], src[k], n * (k == 4 ? 1u : 3u) * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        }
        int rc = enqueue_upsample_prepare(u, u->floor_used);
        if (rc != VK_OK) return rc;
        u->loaded = true; u->loads++; u->last_launches = 1u;
        return VK_OK;
    });
}

int vk_upsample_apply(vk_upsample *u, const vk_upsample_params *p, const float *albedo_hi, const float *normal_hi, const float *depth_hi,
    float *rgb_out, float *stderr3_out) {
    int rc = check_upsample_apply(u, p, albedo_hi, rgb_out, stderr3_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        // (the high guides and the two outputs side by side in the handle's buffer; the guides are uploaded, the outputs come back)
        float *const host[5] = {const_cast<float *>(albedo_hi), const_cast<float *>(normal_hi), const_cast<float *>(depth_hi), rgb_out, stderr3_out};
        const uint32_t comps[5] = {3u, 3u, 1u, 3u, 3u};
        StagedImages im;
        int r = im.upload(u->io, host, comps, 5, upsample_hi(u), 0x7u);
        if (r != VK_OK) return r;
        r = enqueue_upsample(u, *p, im.dev[0], im.dev[1], im.dev[2], im.dev[3], im.dev[4]);
        if (r != VK_OK) return r;
        return im.download(0x18u);                                                        // (waits for the null stream)
    });
}

int vk_upsample_apply_device(vk_upsample *u, const vk_upsample_params *p, const void *d_albedo_hi, const void *d_normal_hi,
    const void *d_depth_hi, void *d_rgb_out, void *d_stderr3_out) {
    int rc = check_upsample_apply(u, p, d_albedo_hi, d_rgb_out, d_stderr3_out);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        return enqueue_upsample(u, *p, static_cast<const float *>(d_albedo_hi), static_cast<const float *>(d_normal_hi),
                                static_cast<const float *>(d_depth_hi), static_cast<float *>(d_rgb_out), static_cast<float *>(d_stderr3_out));
    });
}

int vk_upsample_reset(vk_upsample *u) {
    if (!u) return fail(VK_ERR_BAD_ARG, "null upsample handle");
    u->loaded = false;
    for (float *&at : u->raw_at) at = nullptr;
    return VK_OK;
}

int vk_upsample_get_info(vk_upsample *u, vk_upsample_info *out) {
    if (!u || !out) return fail(VK_ERR_BAD_ARG, "null argument (upsample handle or out)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        double ms = 0.0;
        int rc = upsample_elapsed(u, &ms);
        if (rc != VK_OK) return rc;
        uint32_t counts[2] = {0u, 0u};
        HIP_TRY(hipMemcpy(counts, u->counts, sizeof(counts), hipMemcpyDeviceToHost));     // (waits for the null stream)
        memset(out, 0, sizeof(*out));
        out->width_lo = u->w; out->height_lo = u->h; out->width_hi = u->W; out->height_hi = u->H;
        out->loaded = u->loaded ? 1u : 0u; out->guides = u->loaded ? upsample_guides(u) : 0u;
        out->loads = u->loads; out->applies = u->applies; out->last_form = u->last_form; out->last_launches = u->last_launches;
        out->last_kernel_ms = ms;
        out->scratch_bytes = u->raw.bytes() + u->planes.bytes() + u->counts.bytes() + u->io.bytes();
        out->fallback_pixels = counts[0]; out->empty_pixels = counts[1];
        return VK_OK;
    });
}

void vk_upsample_destroy(vk_upsample *u) {
    if (u) upsample_free(u);
}

// test hook (vecchio_amd_debug.h): the form of the apply's filter kernel
int vk_debug_upsample_set_form(vk_upsample *u, uint32_t form) {
    if (!u) return fail(VK_ERR_BAD_ARG, "null upsample handle");
    if (form > (uint32_t)VK_UPSAMPLE_FORM_TILED) return fail(VK_ERR_BAD_ARG, "unknown upsample form");
    u->form = form;
    return VK_OK;
}

// test hook (vecchio_amd_debug.h): the last apply's filter kernel, from the events recorded around it; 0 before one
int vk_debug_upsample_last_ms(vk_upsample *u, double *ms) {
    if (!u || !ms) return fail(VK_ERR_BAD_ARG, "null argument (upsample handle or ms)");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(first_part(u->scene)->device));
        double got = 0.0;
        int rc = upsample_elapsed(u, &got);
        if (rc != VK_OK) return rc;
        *ms = got;
        return VK_OK;
    });
}

}  // extern "C"

// ---- the denoiser (vk_denoise): denoise_prepare_kernel, then one level kernel per pass (vk_kernels.h), on the scene's device (devices[0]
// of a multi-device scene), on scratch and events of its own: nothing that describes vk_render's last frame is read or written.
namespace {

// Per level the form that was measured faster on the MI355X (tools/denoise_report.py): the staged form up to tap
// spacing 8 (1920x1080: 0.111-0.121 ms against 0.135-0.139 ms a level), the plain form from 16 on (0.132 against 0.149 ms at 16, 0.129
// against 0.200 ms at 32: the halo outgrows the tile).  The staged form exists up to DN_STAGED_MAX_S (48 KB of LDS per workgroup there).
constexpr int DN_STAGED_MAX_S = 32;
constexpr int DN_STAGED_AUTO_MAX_S = 8;
// images of vk_denoise: color, stderr3, albedo, normal, depth, out
constexpr uint32_t DN_COMPONENTS[6] = {3u, 3u, 3u, 3u, 1u, 3u};

int check_denoise_args(vk_scene *scene, const vk_denoise_params *dp, const void *const img[6]) {
    if (!scene || !dp || !img[0] || !img[5]) return fail(VK_ERR_BAD_ARG, "null argument");
    if (dp->width == 0 || dp->height == 0) return fail(VK_ERR_BAD_ARG, "width and height must be >= 1");
    if ((uint64_t)dp->width * dp->height > (1ull << 31) / 3 || dp->width > 65535u || dp->height > 65535u) return fail(VK_ERR_BAD_ARG,
        "image too large");
    if (dp->levels < 1u || dp->levels > 8u) return fail(VK_ERR_BAD_ARG, "levels must be in 1..8");
    if (dp->normal_squarings > 10u) return fail(VK_ERR_BAD_ARG, "normal_squarings must be in 0..10");
    for (float v : {dp->sigma_l, dp->sigma_z, dp->albedo_floor})
        if (!std::isfinite(v) || !(v > 0.0f)) return fail(VK_ERR_BAD_ARG, "sigma_l, sigma_z and albedo_floor must be finite and > 0");
    if (dp->flags != 0u) return fail(VK_ERR_BAD_ARG, "unknown denoise flags");
    const size_t n = (size_t)dp->width * dp->height;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(img[5]), o1 = o0 + n * 3 * sizeof(float);
    for (int k = 0; k < 5; k++) {
        if (!img[k]) continue;
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(img[k]), i1 = i0 + n * DN_COMPONENTS[k] * sizeof(float);
        if (i0 < o1 && o0 < i1) return fail(VK_ERR_BAD_ARG, "out overlaps an input");
    }
    return VK_OK;
}

int enqueue_denoise(vk_scene *q, const vk_denoise_params *dp, const float *const d[6], hipStream_t st, bool timed) {
    HIP_TRY(hipSetDevice(q->device));
    const size_t n = (size_t)dp->width * dp->height;
    int rc = q->dn.buf.ensure(n * (3 * sizeof(float4) + sizeof(float2)));
    if (rc != VK_OK) return rc;
    float4 *P[2] = {reinterpret_cast<float4 *>(q->dn.buf.get()), reinterpret_cast<float4 *>(q->dn.buf.get()) + n};
    DnArgs A;
    memset(&A, 0, sizeof(A));
    A.G = reinterpret_cast<float4 *>(q->dn.buf.get()) + 2 * n;
    A.S = reinterpret_cast<float2 *>(reinterpret_cast<float4 *>(q->dn.buf.get()) + 3 * n);
    A.color = d[0]; A.stderr3 = d[1]; A.albedo = d[2]; A.normal = d[3]; A.depth = d[4]; A.out = const_cast<float *>(d[5]);
    A.width = dp->width; A.height = dp->height; A.normal_squarings = dp->normal_squarings;
    A.sigma_l = dp->sigma_l; A.sigma_z = dp->sigma_z; A.albedo_floor = dp->albedo_floor;
    const uint32_t guides = (d[1] ? DN_HAS_STDERR : 0u) | (d[2] ? DN_HAS_ALBEDO : 0u) | (d[3] ? DN_HAS_NORMAL : 0u) | (d[4] ? DN_HAS_DEPTH : 0u);
    if (timed) {
        for (uint32_t k = 0; k < dp->levels + 2u; k++) if ((rc = q->dn.ev[k].create()) != VK_OK) return rc;
        HIP_TRY(hipEventRecord(q->dn.ev[0], st));
    }
    const dim3 grid((dp->width + DN_SX - 1) / DN_SX, (dp->height + DN_R - 1) / DN_R);
    A.flags = guides; A.Pout = P[0]; A.s = 1;
    hipLaunchKernelGGL(denoise_prepare_kernel, grid, dim3(DN_BLOCK), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(q->dn.ev[1], st));
    for (uint32_t i = 0; i < dp->levels; i++) {
        A.s = 1 << i;
        A.Pin = P[i & 1u]; A.Pout = P[(i & 1u) ^ 1u];
        A.flags = guides | (i + 1u == dp->levels ? DN_LAST : 0u);
        const bool staged = q->dn.form == VK_DENOISE_FORM_PLAIN ? false
            : A.s <= (q->dn.form == VK_DENOISE_FORM_STAGED ? DN_STAGED_MAX_S : DN_STAGED_AUTO_MAX_S);
        if (staged) {
            // one workgroup per DN_SX columns and DN_R rows of one residue class of y mod s
            const uint32_t per_class = ((dp->height + (uint32_t)A.s - 1u) / (uint32_t)A.s + DN_R - 1) / DN_R;
            hipLaunchKernelGGL(denoise_level_staged_kernel, dim3(grid.x, (uint32_t)A.s * per_class), dim3(DN_BLOCK), dn_staged_lds_bytes(A.s),
                               st, A);
        } else {
            hipLaunchKernelGGL(denoise_level_plain_kernel, grid, dim3(DN_BLOCK), 0, st, A);
        }
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(q->dn.ev[2 + i], st));
    }
    if (timed) q->dn.last_levels = dp->levels;
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_denoise_default_params(uint32_t width, uint32_t height, vk_denoise_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->width = width; out->height = height;
    out->levels = 5u; out->normal_squarings = 7u;
    out->sigma_l = 4.0f; out->sigma_z = 1.0f; out->albedo_floor = 1e-3f;
    return VK_OK;
}

int vk_denoise(vk_scene *scene, const vk_denoise_params *dp, const float *color, const float *stderr3, const float *albedo,
    const float *normal, const float *depth, float *out, vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *const host[6] = {const_cast<float *>(color), const_cast<float *>(stderr3), const_cast<float *>(albedo),
                                const_cast<float *>(normal), const_cast<float *>(depth), out};
        int rc = check_denoise_args(scene, dp, reinterpret_cast<const void *const *>(host));
        if (rc != VK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        vk_scene *q = first_part(scene);
        HIP_TRY(hipSetDevice(q->device));
        const size_t n = (size_t)dp->width * dp->height;
        StagedImages im;
        if ((rc = im.upload(q->dn.io, host, DN_COMPONENTS, 6, n, 0x1Fu)) != VK_OK) return rc;      // (every image but out)
        if ((rc = enqueue_denoise(q, dp, im.dev, nullptr, true)) != VK_OK) return rc;
        if ((rc = im.download(1u << 5)) != VK_OK) return rc;
        if (stats_out) {
            memset(stats_out, 0, sizeof(*stats_out));
            stats_out->samples = n;
            stats_out->kernel_launches = 1u + dp->levels;
        }
        return end_timed_call(q->dn.ev[0], q->dn.ev[1 + dp->levels], t0, stats_out);
    });
}

int vk_denoise_device(vk_scene *scene, const vk_denoise_params *dp, const void *d_color, const void *d_stderr3, const void *d_albedo,
    const void *d_normal, const void *d_depth, void *d_out, void *hip_stream) {
    return guarded([&]() -> int {
        const float *dev[6] = {static_cast<const float *>(d_color), static_cast<const float *>(d_stderr3), static_cast<const float *>(d_albedo),
                               static_cast<const float *>(d_normal), static_cast<const float *>(d_depth), static_cast<const float *>(d_out)};
        int rc = check_denoise_args(scene, dp, reinterpret_cast<const void *const *>(dev));
        if (rc != VK_OK) return rc;
        vk_scene *q = first_part(scene);
        return enqueue_denoise(q, dp, dev, reinterpret_cast<hipStream_t>(hip_stream), false);
    });
}

int vk_debug_denoise_form(vk_scene *scene, int form) {
    if (!scene) return fail(VK_ERR_BAD_ARG, "null scene");
    if (form < VK_DENOISE_FORM_AUTO || form > VK_DENOISE_FORM_STAGED) return fail(VK_ERR_BAD_ARG, "unknown denoise form");
    first_part(scene)->dn.form = form;
    return VK_OK;
}

int vk_debug_denoise_last_ms(vk_scene *scene, double ms_out[9]) {
    if (!scene || !ms_out) return fail(VK_ERR_BAD_ARG, "null argument");
    vk_scene *q = first_part(scene);
    if (q->dn.last_levels == 0u) return fail(VK_ERR_BAD_ARG, "no vk_denoise on this scene yet");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(q->device));
        HIP_TRY(hipEventSynchronize(q->dn.ev[1 + q->dn.last_levels]));
        for (uint32_t k = 0; k < 9u; k++) {
            float ms = 0.0f;
            if (k <= q->dn.last_levels) HIP_TRY(hipEventElapsedTime(&ms, q->dn.ev[k], q->dn.ev[k + 1]));
            ms_out[k] = (double)ms;
        }
        return VK_OK;
    });
}

}  // extern "C"

// ---- temporal accumulation (vk_temporal_*): temporal_accumulate_kernel (vk_kernels.h) on the scene's device (devices[0] of a
// multi-device scene).  The handle owns everything it touches: the two histories, the device copies of the host call's images, the
// counter and its events; nothing of the scene handle is read but its device.
struct vk_temporal {
    int device = 0;
    vk_temporal_params tp{};
    DeviceBuffer<float4> hist;                      // two histories of three planes of width*height float4 each
    DeviceBuffer<unsigned long long> count;         // pixels_with_history of the last frame
    DeviceBuffer<float> io;                         // vk_temporal_accumulate's images on the device
    Event ev0, ev1;                                 // around the last frame's kernel (ev1: what vk_temporal_get_info waits for)
    uint32_t frames = 0;                            // since create or reset
    uint32_t cur = 0;                               // the history the last frame wrote
    vk_camera prev{};                               // the last frame's camera
};

namespace {

// images of vk_temporal_accumulate: color, stderr3, albedo, normal, depth, out_color, out_stderr3, out_history
constexpr uint32_t TA_COMPONENTS[8] = {3u, 3u, 3u, 3u, 1u, 3u, 3u, 1u};

int check_temporal_params(const vk_temporal_params *tp) {
    if (tp->width < 2u || tp->height < 2u) return fail(VK_ERR_BAD_ARG, "width and height must be >= 2");
    if ((uint64_t)tp->width * tp->height > (1ull << 31) / 3 || tp->width > 65535u || tp->height > 65535u) return fail(VK_ERR_BAD_ARG,
        "image too large");
    if (tp->max_history < 1u || tp->max_history > 65535u) return fail(VK_ERR_BAD_ARG, "max_history must be in 1..65535");
    if (!std::isfinite(tp->depth_tol) || !(tp->depth_tol > 0.0f)) return fail(VK_ERR_BAD_ARG, "depth_tol must be finite and > 0");
    if (!std::isfinite(tp->normal_cos_min) || !(tp->normal_cos_min >= -1.0f && tp->normal_cos_min <= 1.0f)) return fail(VK_ERR_BAD_ARG,
        "normal_cos_min must be finite and in -1..1");
    if (!std::isfinite(tp->albedo_floor) || !(tp->albedo_floor > 0.0f)) return fail(VK_ERR_BAD_ARG, "albedo_floor must be finite and > 0");
    if (tp->flags != 0u) return fail(VK_ERR_BAD_ARG, "unknown temporal flags");
    return VK_OK;
}

int check_temporal_args(vk_temporal *t, const vk_camera *cam, const void *const img[8]) {
    if (!t || !cam || !img[0] || !img[3] || !img[4] || !img[5]) return fail(VK_ERR_BAD_ARG, "null argument");
    if (img[6] && !img[1]) return fail(VK_ERR_BAD_ARG, "out_stderr3 needs stderr3");
    const size_t n = (size_t)t->tp.width * t->tp.height;
    for (int k = 5; k < 8; k++) {
        if (!img[k]) continue;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(img[k]), o1 = o0 + n * TA_COMPONENTS[k] * sizeof(float);
        for (int j = 0; j < k; j++) {
            if (!img[j]) continue;
            const uintptr_t i0 = reinterpret_cast<uintptr_t>(img[j]), i1 = i0 + n * TA_COMPONENTS[j] * sizeof(float);
            if (i0 < o1 && o0 < i1) return fail(VK_ERR_BAD_ARG, "an output overlaps an input or another output");
        }
    }
    return VK_OK;
}

inline float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

int enqueue_temporal(vk_temporal *t, const vk_camera *cam, const float *const d[8], hipStream_t st, bool timed) {
    HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)t->tp.width * t->tp.height;
    const uint32_t next = t->cur ^ 1u;
    TaArgs A;
    memset(&A, 0, sizeof(A));
    A.Hin = t->hist + (size_t)t->cur * 3 * n; A.Hout = t->hist + (size_t)next * 3 * n;
    A.color = d[0]; A.stderr3 = d[1]; A.albedo = d[2]; A.normal = d[3]; A.depth = d[4];
    A.out_color = const_cast<float *>(d[5]); A.out_stderr3 = const_cast<float *>(d[6]); A.out_history = const_cast<float *>(d[7]);
    A.count = t->count;
    A.width = t->tp.width; A.height = t->tp.height;
    A.flags = (d[1] ? TA_HAS_STDERR : 0u) | (d[2] ? TA_HAS_ALBEDO : 0u) | (t->frames > 0u ? TA_HAS_HISTORY : 0u);
    A.max_history = (float)t->tp.max_history; A.depth_tol = t->tp.depth_tol; A.normal_cos_min = t->tp.normal_cos_min;
    A.albedo_floor = t->tp.albedo_floor;
    const vk_camera &c = *cam, &pc = t->prev;
    for (int k = 0; k < 3; k++) {
        A.o[k] = c.origin[k]; A.llc[k] = c.lower_left_corner[k]; A.H[k] = c.horizontal[k]; A.V[k] = c.vertical[k];
        A.po[k] = pc.origin[k]; A.pq[k] = pc.lower_left_corner[k] - pc.origin[k]; A.pw[k] = pc.w[k];
        A.pH[k] = pc.horizontal[k]; A.pV[k] = pc.vertical[k];
    }
    A.fw = -dot3(A.pq, A.pw); A.HH = dot3(A.pH, A.pH); A.VV = dot3(A.pV, A.pV);
    HIP_TRY(hipMemsetAsync(t->count, 0, sizeof(unsigned long long), st));
    if (timed) HIP_TRY(hipEventRecord(t->ev0, st));
    const dim3 grid((t->tp.width + DN_SX - 1) / DN_SX, (t->tp.height + DN_R - 1) / DN_R);
    hipLaunchKernelGGL(temporal_accumulate_kernel, grid, dim3(DN_BLOCK), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev1, st));
    t->cur = next; t->frames++; t->prev = *cam;
    return VK_OK;
}

void temporal_free(vk_temporal *t) {
    (void)hipSetDevice(t->device);
    if (t->ev1) (void)hipEventSynchronize(t->ev1);
    delete t;
}

}  // namespace

extern "C" {

int vk_temporal_default_params(uint32_t width, uint32_t height, vk_temporal_params *out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->width = width; out->height = height;
    out->max_history = 32u; out->depth_tol = 0.02f; out->normal_cos_min = 0.9f; out->albedo_floor = 1e-3f;
    return VK_OK;
}

int vk_temporal_create(vk_scene *scene, const vk_temporal_params *tp, vk_temporal **out) {
    if (!tp || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    int rc = check_temporal_params(tp);
    if (rc != VK_OK) return rc;
    if (!scene) return fail(VK_ERR_BAD_ARG, "null scene");
    return guarded([&]() -> int {
        std::unique_ptr<vk_temporal, void (*)(vk_temporal *)> t(new vk_temporal(), temporal_free);
        t->device = first_part(scene)->device;
        t->tp = *tp;
        const size_t n = (size_t)tp->width * tp->height;
        HIP_TRY(hipSetDevice(t->device));
        hipError_t e;      // (out of device memory has a code of its own)
        if ((e = t->hist.alloc(6 * n * sizeof(float4))) != hipSuccess) return fail(e == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP,
            std::string("hipMalloc (history): ") + hipGetErrorString(e));
        if ((e = t->count.alloc(sizeof(unsigned long long))) != hipSuccess) return fail(e == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP,
            std::string("hipMalloc: ") + hipGetErrorString(e));
        int rc;
        HIP_TRY(hipMemset(t->count, 0, sizeof(unsigned long long)));
        if ((rc = t->ev0.create()) != VK_OK || (rc = t->ev1.create()) != VK_OK) return rc;
        *out = t.release();
        return VK_OK;
    });
}

int vk_temporal_accumulate(vk_temporal *t, const vk_camera *cam, const float *color, const float *stderr3, const float *albedo,
    const float *normal, const float *depth, float *out_color, float *out_stderr3, float *out_history, vk_stats *stats_out) {
    return guarded([&]() -> int {
        float *const host[8] = {const_cast<float *>(color), const_cast<float *>(stderr3), const_cast<float *>(albedo),
                                const_cast<float *>(normal), const_cast<float *>(depth), out_color, out_stderr3, out_history};
        int rc = check_temporal_args(t, cam, reinterpret_cast<const void *const *>(host));
        if (rc != VK_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(t->device));
        const size_t n = (size_t)t->tp.width * t->tp.height;
        StagedImages im;
        if ((rc = im.upload(t->io, host, TA_COMPONENTS, 8, n, 0x1Fu)) != VK_OK) return rc;      // (the inputs)
        if ((rc = enqueue_temporal(t, cam, im.dev, nullptr, true)) != VK_OK) return rc;
        if ((rc = im.download(0xE0u)) != VK_OK) return rc;                                      // (the three outputs)
        if (stats_out) {
            memset(stats_out, 0, sizeof(*stats_out));
            stats_out->samples = n;
            stats_out->kernel_launches = 1u;
        }
        return end_timed_call(t->ev0, t->ev1, t0, stats_out);
    });
}

int vk_temporal_accumulate_device(vk_temporal *t, const vk_camera *cam, const void *d_color, const void *d_stderr3, const void *d_albedo,
    const void *d_normal, const void *d_depth, void *d_out_color, void *d_out_stderr3, void *d_out_history, void *hip_stream) {
    return guarded([&]() -> int {
        const float *dev[8] = {static_cast<const float *>(d_color), static_cast<const float *>(d_stderr3), static_cast<const float *>(d_albedo),
                               static_cast<const float *>(d_normal), static_cast<const float *>(d_depth), static_cast<const float *>(d_out_color),
                               static_cast<const float *>(d_out_stderr3), static_cast<const float *>(d_out_history)};
        int rc = check_temporal_args(t, cam, reinterpret_cast<const void *const *>(dev));
        if (rc != VK_OK) return rc;
        return enqueue_temporal(t, cam, dev, reinterpret_cast<hipStream_t>(hip_stream), false);
    });
}

int vk_temporal_reset(vk_temporal *t) {
    if (!t) return fail(VK_ERR_BAD_ARG, "null temporal handle");
    t->frames = 0;                                   // (the histories stay where they are: a first frame reads none)
    return VK_OK;
}

int vk_temporal_get_info(vk_temporal *t, vk_temporal_info *out) {
    if (!t || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    return guarded([&]() -> int {
        memset(out, 0, sizeof(*out));
        out->frames = t->frames; out->width = t->tp.width; out->height = t->tp.height;
        if (t->frames > 0u) {
            unsigned long long c = 0;
            HIP_TRY(hipSetDevice(t->device));
            HIP_TRY(hipEventSynchronize(t->ev1));
            HIP_TRY(hipMemcpy(&c, t->count, sizeof(c), hipMemcpyDeviceToHost));
            out->pixels_with_history = c;
        }
        return VK_OK;
    });
}

void vk_temporal_destroy(vk_temporal *t) {
    if (t) temporal_free(t);
}

}  // extern "C"

// ---- progressive rendering (ABI 7): one camera + one vk_render_params, running sums on every device part of the scene.  A step is an
// ordinary render of the sample window [done, done + n) (KArgs::sample_base) whose resolve is replaced by accumulate_resolve_kernel.
struct vk_progress {
    vk_scene *scene = nullptr;
    vk_camera cam;
    vk_render_params params;       // samples_per_pixel = the budget
    uint32_t flags = 0, done = 0, steps = 0;
    bool adaptive = false;         // vk_progress_set_adaptive
    vk_adaptive_params ap;
    struct Part {                  // one per device part (the scene itself for a one-device scene)
        int device = 0;
        DeviceBuffer<long long> run;
        DeviceBuffer<double> m2;
        DeviceBuffer<unsigned long long> clamped;
        Event ev;
        // the part's share of the partition: tiles rank + world * i, i < n_local (in_px: their in-image pixels)
        uint32_t rank = 0, world = 1, n_local = 0;
        uint64_t in_px = 0;
        // adaptive (allocated by vk_progress_set_adaptive): see AccumDesc
        DeviceBuffer<uint32_t> tile_n, tile_k, list, ctl;
        PinnedBuffer<uint32_t> h_left;
    };
    std::vector<Part> parts;
    size_t n_words = 0;            // width*height*3
};

namespace {

// an allocation of a progressive handle: any failure counts as out of memory (the sticky error cleared)
template <class T>
bool device_alloc(DeviceBuffer<T> &b, size_t bytes) {
    if (b.alloc(bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// (waits for each part's last step before the part's sums go)
void progress_free(vk_progress *pr) {
    for (auto &q : pr->parts) {
        (void)hipSetDevice(q.device);
        if (q.ev) (void)hipEventSynchronize(q.ev);
    }
    (void)hipGetLastError();
    delete pr;
}

// waits for the handle's last step on every part
int progress_wait(vk_progress *pr) {
    for (auto &q : pr->parts) {
        HIP_TRY(hipSetDevice(q.device));
        HIP_TRY(hipEventSynchronize(q.ev));
    }
    return VK_OK;
}

// adaptive: every tile active again, and the host's counts those of the whole share (after the last step)
int progress_zero_tiles(vk_progress *pr) {
    for (auto &q : pr->parts) {
        if (!q.tile_n) continue;
        HIP_TRY(hipSetDevice(q.device));
        HIP_TRY(hipMemset(q.tile_n, 0, (size_t)q.n_local * sizeof(uint32_t) + 4));
        HIP_TRY(hipMemset(q.tile_k, 0, (size_t)q.n_local * sizeof(uint32_t) + 4));
        HIP_TRY(hipDeviceSynchronize());
        q.h_left[0] = q.n_local;
        memcpy(q.h_left + 1, &q.in_px, sizeof(uint64_t));
    }
    return VK_OK;
}

// back to sample 0: the running sums, error moments and clamped count := 0 (after the last step, before anything later)
int progress_zero(vk_progress *pr) {
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    for (auto &q : pr->parts) {
        HIP_TRY(hipSetDevice(q.device));
        HIP_TRY(hipMemset(q.run, 0, pr->n_words * sizeof(long long)));
        if (q.m2) HIP_TRY(hipMemset(q.m2, 0, pr->n_words * sizeof(double)));
        HIP_TRY(hipMemset(q.clamped, 0, sizeof(unsigned long long)));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipEventRecord(q.ev, nullptr));      // (progress_wait has an event to wait for before the first step)
    }
    rc = progress_zero_tiles(pr);
    if (rc != VK_OK) return rc;
    pr->done = 0; pr->steps = 0;
    return VK_OK;
}

// the argument checks of a step (nothing is enqueued, the handle is not touched when one fails); pw = the window's params
int progress_step_args(vk_progress *pr, uint32_t n, vk_render_params &pw) {
    if (!pr) return fail(VK_ERR_BAD_ARG, "null progress handle");
    if (n == 0) return fail(VK_ERR_BAD_ARG, "n_samples must be >= 1");
    if ((uint64_t)pr->done + n > pr->params.samples_per_pixel) return fail(VK_ERR_BAD_ARG, "samples_done + n_samples exceeds the budget");
    pw = pr->params;
    pw.samples_per_pixel = n;
    return check_render_args(pr->scene, &pr->cam, &pw);
}

// the active tiles and their pixels after the last window whose counts have landed in h_left (wait: the last step's); else the share's
void progress_known(const vk_progress::Part &q, bool wait, AccumDesc &d) {
    bool landed = wait ? hipEventSynchronize(q.ev) == hipSuccess : hipEventQuery(q.ev) == hipSuccess;
    (void)hipGetLastError();
    d.known_tiles = q.n_local; d.known_px = q.in_px;
    if (landed) { d.known_tiles = q.h_left[0]; memcpy(&d.known_px, q.h_left + 1, sizeof(uint64_t)); }
}

std::vector<AccumDesc> progress_descs(vk_progress *pr, uint32_t n, bool wait) {
    std::vector<AccumDesc> d(pr->parts.size());
    for (size_t j = 0; j < d.size(); j++) {
        const auto &q = pr->parts[j];
        memset(&d[j], 0, sizeof(AccumDesc));
        d[j].sample_base = pr->done; d[j].budget = pr->params.samples_per_pixel; d[j].done = pr->done + n;
        d[j].run = q.run; d[j].m2 = q.m2; d[j].clamped = q.clamped; d[j].ev_done = q.ev;
        if (pr->adaptive) {
            (void)hipSetDevice(q.device);
            d[j].tile_n = q.tile_n; d[j].tile_k = q.tile_k; d[j].list = q.list; d[j].ctl = q.ctl; d[j].h_left = q.h_left;
            d[j].steps = pr->steps + 1;
            d[j].gate = (d[j].done >= pr->ap.min_samples && d[j].steps >= pr->ap.min_steps) ? 1u : 0u;
            d[j].abs_tol = pr->ap.abs_tol; d[j].rel_tol = pr->ap.rel_tol;
            progress_known(q, wait, d[j]);
        }
    }
    return d;
}

// per tile of the image (row-major, row 0 at the bottom): samples and windows in its running sums (0, 0 outside the partition).  After
// the last step.
int progress_tile_map(vk_progress *pr, std::vector<uint32_t> &n, std::vector<uint32_t> &k, uint32_t *n_active = nullptr) {
    const TileGeom g(&pr->params);
    n.assign(g.tiles, 0u); k.assign(g.tiles, 0u);
    if (n_active) *n_active = 0;
    for (auto &q : pr->parts) {
        std::vector<uint32_t> tn(q.n_local, 0u), tk(q.n_local, 0u);
        if (q.tile_n && q.n_local) {
            HIP_TRY(hipSetDevice(q.device));
            HIP_TRY(hipMemcpy(tn.data(), q.tile_n, q.n_local * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(tk.data(), q.tile_k, q.n_local * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        for (uint32_t i = 0; i < q.n_local; i++) {
            const uint32_t t = q.rank + i * q.world;
            n[t] = tn[i] ? tn[i] : pr->done; k[t] = tn[i] ? tk[i] : pr->steps;
            if (n_active && tn[i] == 0u) ++*n_active;
        }
    }
    return VK_OK;
}

}  // namespace

extern "C" {

int vk_progress_create(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t flags, vk_progress **out) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)VK_PROGRESS_STDERR) return fail(VK_ERR_BAD_ARG, "unknown progress flags");
    int rc = check_render_args(scene, cam, params);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        std::unique_ptr<vk_progress, void (*)(vk_progress *)> pr(new vk_progress, progress_free);
        pr->scene = scene; pr->cam = *cam; pr->params = *params; pr->flags = flags;
        memset(&pr->ap, 0, sizeof(pr->ap));
        pr->n_words = (size_t)params->width * params->height * 3;
        std::vector<vk_scene *> parts = scene->group.parts;
        if (parts.empty()) parts.push_back(scene);
        const TileGeom g(params);
        for (size_t j = 0; j < parts.size(); j++) {
            vk_scene *q = parts[j];
            pr->parts.emplace_back();
            auto &P = pr->parts.back();
            P.device = q->device;
            // (enqueue_render_multi's split: part j of n renders tiles R + W (j + n i))
            vk_render_params pj = *params;
            pj.tile_rank = g.rank + g.world * (uint32_t)j; pj.tile_world = g.world * (uint32_t)parts.size();
            const TileGeom gj(&pj);
            P.rank = gj.rank; P.world = gj.world; P.n_local = gj.n_local;
            pj.samples_per_pixel = 1;
            P.in_px = gj.n_local ? partition_samples(&pj, gj) : 0u;
            if (hipSetDevice(q->device) != hipSuccess) return fail(VK_ERR_HIP, "hipSetDevice failed");
            if (!device_alloc(P.run, pr->n_words * sizeof(long long)) || ((flags & VK_PROGRESS_STDERR) && !device_alloc(P.m2, pr->n_words * sizeof(double))) ||
                !device_alloc(P.clamped, sizeof(unsigned long long))) return fail(VK_ERR_OOM, "out of device memory");
            if (P.ev.create(hipEventDisableTiming) != VK_OK) return fail(VK_ERR_HIP, "hipEventCreate failed");
        }
        int z = progress_zero(pr.get());
        if (z != VK_OK) return z;
        *out = pr.release();
        return VK_OK;
    });
}

int vk_progress_set_adaptive(vk_progress *pr, const vk_adaptive_params *ap) {
    if (!pr || !ap) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!(pr->flags & VK_PROGRESS_STDERR)) return fail(VK_ERR_BAD_ARG, "adaptive sampling judges the error moments: it needs VK_PROGRESS_STDERR");
    if (pr->steps != 0) return fail(VK_ERR_BAD_ARG, "adaptive sampling is set before the first step since create / reset");
    if (ap->min_steps < 2) return fail(VK_ERR_BAD_ARG, "min_steps must be >= 2 (the error estimate needs two windows)");
    if (!(std::isfinite(ap->abs_tol) && ap->abs_tol >= 0.0f && std::isfinite(ap->rel_tol) && ap->rel_tol >= 0.0f))
        return fail(VK_ERR_BAD_ARG, "abs_tol and rel_tol must be finite and >= 0");
    return guarded([&]() -> int {
        int rc = progress_wait(pr);
        if (rc != VK_OK) return rc;
        for (auto &q : pr->parts) {
            if (q.tile_n) continue;
            HIP_TRY(hipSetDevice(q.device));
            const size_t words = (size_t)q.n_local + 1u;
            int e = VK_OK;
            if (!device_alloc(q.tile_n, words * sizeof(uint32_t)) || !device_alloc(q.tile_k, words * sizeof(uint32_t)) ||
                !device_alloc(q.list, words * sizeof(uint32_t)) || !device_alloc(q.ctl, (4u + (q.n_local + 1023u) / 1024u) * sizeof(uint32_t)))
                e = fail(VK_ERR_OOM, "out of device memory");
            else if (q.h_left.alloc(4 * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); e = fail(VK_ERR_OOM, "out of pinned host memory"); }
            if (e != VK_OK) {      // (the handle as it was: non-adaptive, nothing of this call kept)
                for (auto &u : pr->parts) { u.tile_n.reset(); u.tile_k.reset(); u.list.reset(); u.ctl.reset(); u.h_left.reset(); }
                return e;
            }
        }
        rc = progress_zero_tiles(pr);
        if (rc != VK_OK) return rc;
        pr->ap = *ap;
        pr->adaptive = true;
        return VK_OK;
    });
}

int vk_progress_step(vk_progress *pr, uint32_t n_samples, void *out, vk_stats *stats_out) {
    vk_render_params pw;
    int rc = progress_step_args(pr, n_samples, pw);
    if (rc != VK_OK) return rc;
    if (!out) return fail(VK_ERR_BAD_ARG, "null framebuffer");
    return guarded([&]() -> int {
        const std::vector<AccumDesc> d = progress_descs(pr, n_samples, true);     // (adaptive: the exact active counts of this window)
        int r = render_host(pr->scene, &pr->cam, &pw, out, stats_out, nullptr, d.data());
        if (r != VK_OK) return r;
        pr->done += n_samples; pr->steps++;
        return VK_OK;
    });
}

int vk_progress_step_device(vk_progress *pr, uint32_t n_samples, void *d_out, void *hip_stream, vk_stats *stats_out) {
    vk_render_params pw;
    int rc = progress_step_args(pr, n_samples, pw);
    if (rc != VK_OK) return rc;
    if (!d_out) return fail(VK_ERR_BAD_ARG, "null framebuffer");
    return guarded([&]() -> int {
        const std::vector<AccumDesc> d = progress_descs(pr, n_samples, false);    // (never waits: counts as far as the host knows)
        int r = enqueue_render(pr->scene, &pr->cam, &pw, d_out, reinterpret_cast<hipStream_t>(hip_stream), false, stats_out, d.data());
        if (r != VK_OK) return r;
        pr->done += n_samples; pr->steps++;
        return VK_OK;
    });
}

int vk_progress_reset(vk_progress *pr, const vk_camera *cam) {
    if (!pr) return fail(VK_ERR_BAD_ARG, "null progress handle");
    if (cam) {
        int rc = check_render_args(pr->scene, cam, &pr->params);
        if (rc != VK_OK) return rc;
    }
    return guarded([&]() -> int {
        int rc = progress_zero(pr);
        if (rc != VK_OK) return rc;
        if (cam) pr->cam = *cam;
        return VK_OK;
    });
}

int vk_progress_get_info(vk_progress *pr, vk_progress_info *out) {
    if (!pr || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    uint64_t clamped = 0;
    for (auto &q : pr->parts) {
        unsigned long long v = 0;
        HIP_TRY(hipSetDevice(q.device));
        HIP_TRY(hipMemcpy(&v, q.clamped, sizeof(v), hipMemcpyDeviceToHost));
        clamped += v;
    }
    out->samples_done = pr->done; out->samples_budget = pr->params.samples_per_pixel; out->steps = pr->steps; out->flags = pr->flags;
    out->clamped_samples = clamped;
    return VK_OK;
}

int vk_progress_tile_samples(vk_progress *pr, uint32_t *out, vk_adaptive_info *info) {
    if (!pr) return fail(VK_ERR_BAD_ARG, "null progress handle");
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        std::vector<uint32_t> n, k;
        uint32_t active = 0;
        int r = progress_tile_map(pr, n, k, &active);
        if (r != VK_OK) return r;
        if (out) memcpy(out, n.data(), n.size() * sizeof(uint32_t));
        if (info) {
            const vk_render_params &p = pr->params;
            const TileGeom g(&p);
            memset(info, 0, sizeof(*info));
            for (uint32_t t = g.rank; t < g.tiles; t += g.world) {
                const uint32_t tx = (t % g.tiles_x) * TILE, ty = (t / g.tiles_x) * TILE;
                const uint64_t px = (uint64_t)std::min<uint32_t>(TILE, p.width - tx) * std::min<uint32_t>(TILE, p.height - ty);
                info->tiles_total++;
                info->samples_rendered += px * n[t];
            }
            info->tiles_active = active;
        }
        return VK_OK;
    });
}

// Batch means over the steps (not on the hot path): per component sqrt((sum_j n_j m_j^2 - N m^2) / ((k - 1) N)).  The parts' sums are
// zero outside their own tiles, so the whole partition's are their sum.  Adaptive: N and k are each tile's own.
int vk_progress_stderr(vk_progress *pr, float *out) {
    if (!pr || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!(pr->flags & VK_PROGRESS_STDERR)) return fail(VK_ERR_BAD_ARG, "the handle was created without VK_PROGRESS_STDERR");
    if (pr->steps < 2) return fail(VK_ERR_BAD_ARG, "the standard error needs two steps or more");
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        std::vector<long long> run(pr->n_words, 0), r(pr->n_words);
        std::vector<double> m2(pr->n_words, 0.0), m(pr->n_words);
        for (auto &q : pr->parts) {
            HIP_TRY(hipSetDevice(q.device));
            HIP_TRY(hipMemcpy(r.data(), q.run, pr->n_words * sizeof(long long), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(m.data(), q.m2, pr->n_words * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < pr->n_words; i++) { run[i] += r[i]; m2[i] += m[i]; }
        }
        std::vector<uint32_t> tn, tk;
        int e = progress_tile_map(pr, tn, tk);
        if (e != VK_OK) return e;
        const vk_render_params &p = pr->params;
        const uint32_t world = p.tile_world ? p.tile_world : 1u, tiles_x = (p.width + TILE - 1) / TILE;
        for (uint32_t y = 0; y < p.height; y++)
            for (uint32_t x = 0; x < p.width; x++) {
                const uint32_t t = (y / TILE) * tiles_x + x / TILE;
                if (t % world != p.tile_rank) continue;
                const double N = (double)tn[t], k = (double)tk[t];
                for (int c = 0; c < 3; c++) {
                    const size_t i = ((size_t)y * p.width + x) * 3 + c;
                    const double mean = (double)run[i] / (double)ACCUM_SCALE / N;
                    const double v = (m2[i] - N * mean * mean) / ((k - 1.0) * N);
                    out[i] = (float)sqrt(v > 0.0 ? v : 0.0);
                }
            }
        return VK_OK;
    });
}

// the same on the device (progress_stderr_kernel), for a handle whose moments live on one device
int vk_progress_stderr_device(vk_progress *pr, void *d_out, void *hip_stream) {
    if (!pr || !d_out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (!(pr->flags & VK_PROGRESS_STDERR)) return fail(VK_ERR_BAD_ARG, "the handle was created without VK_PROGRESS_STDERR");
    if (pr->steps < 2) return fail(VK_ERR_BAD_ARG, "the standard error needs two steps or more");
    if (pr->parts.size() != 1) return fail(VK_ERR_UNSUPPORTED,
        "the handle's moments live on several devices: use vk_progress_stderr (host) on a multi-device scene");
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        const auto &q = pr->parts[0];
        const vk_render_params &p = pr->params;
        HIP_TRY(hipSetDevice(q.device));
        const size_t n = (size_t)p.width * p.height;
        hipLaunchKernelGGL(progress_stderr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                           (const long long *)q.run, (const double *)q.m2, (const uint32_t *)q.tile_n, (const uint32_t *)q.tile_k, pr->done,
                           pr->steps, p.width, p.height, (p.width + TILE - 1) / TILE, q.rank, q.world, static_cast<float *>(d_out));
        HIP_TRY(hipGetLastError());
        return VK_OK;
    });
}

// the raw running sums and error moments, summed over the parts (tests: the judge's inputs)
int vk_debug_progress_moments(vk_progress *pr, long long *run_out, double *m2_out) {
    if (!pr) return fail(VK_ERR_BAD_ARG, "null progress handle");
    if (m2_out && !(pr->flags & VK_PROGRESS_STDERR)) return fail(VK_ERR_BAD_ARG, "the handle was created without VK_PROGRESS_STDERR");
    int rc = progress_wait(pr);
    if (rc != VK_OK) return rc;
    return guarded([&]() -> int {
        std::vector<long long> r(pr->n_words);
        std::vector<double> m(pr->n_words);
        if (run_out) memset(run_out, 0, pr->n_words * sizeof(long long));
        if (m2_out) memset(m2_out, 0, pr->n_words * sizeof(double));
        for (auto &q : pr->parts) {
            HIP_TRY(hipSetDevice(q.device));
            if (run_out) {
                HIP_TRY(hipMemcpy(r.data(), q.run, pr->n_words * sizeof(long long), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < pr->n_words; i++) run_out[i] += r[i];
            }
            if (m2_out) {
                HIP_TRY(hipMemcpy(m.data(), q.m2, pr->n_words * sizeof(double), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < pr->n_words; i++) m2_out[i] += m[i];
            }
        }
        return VK_OK;
    });
}

void vk_progress_destroy(vk_progress *pr) {
    if (pr) progress_free(pr);
}

size_t vk_tile_slab_bytes(uint32_t width, uint32_t height, uint32_t output_format, uint32_t tile_rank, uint32_t tile_world) {
    if (width == 0 || height == 0 || output_format > VK_OUTPUT_RGB8) return 0;
    vk_render_params p; memset(&p, 0, sizeof(p));
    p.width = width; p.height = height; p.tile_world = tile_world ? tile_world : 1u;
    p.tile_rank = tile_rank < p.tile_world ? tile_rank : 0u;       // (rank 0 holds the most tiles)
    return (size_t)TileGeom(&p).n_local * 64u * (output_format == VK_OUTPUT_RGB8 ? 3u : 12u);
}

static int tile_call_args(vk_scene *scene, const void *a, const void *b, uint32_t width, uint32_t height, uint32_t output_format,
    uint32_t tile_rank, uint32_t tile_world, vk_render_params &p) {
    if (!scene || !a || !b) return fail(VK_ERR_BAD_ARG, "null argument");
    if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 31) / 3 || width > 65535u || height > 65535u) return fail(VK_ERR_BAD_ARG,
        "image too large");
    if (output_format > VK_OUTPUT_RGB8) return fail(VK_ERR_BAD_ARG, "bad output_format");
    memset(&p, 0, sizeof(p));
    p.width = width; p.height = height; p.tile_world = tile_world ? tile_world : 1u; p.tile_rank = tile_rank;
    if (p.tile_rank >= p.tile_world) return fail(VK_ERR_BAD_ARG, "tile_rank >= tile_world");
    return VK_OK;
}

int vk_pack_tiles_device(vk_scene *scene, const void *d_fb, uint32_t width, uint32_t height, uint32_t output_format, uint32_t tile_rank,
    uint32_t tile_world, void *d_slab, void *hip_stream) {
    vk_render_params p;
    int rc = tile_call_args(scene, d_fb, d_slab, width, height, output_format, tile_rank, tile_world, p);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return output_format == VK_OUTPUT_RGB8 ? tile_move<TM_PACK_U8>(d_fb, d_slab, &p, TileGeom(&p), st)
                                           : tile_move<TM_PACK_F32>(d_fb, d_slab, &p, TileGeom(&p), st);
}

int vk_unpack_tiles_device(vk_scene *scene, const void *d_slab, uint32_t width, uint32_t height, uint32_t output_format, uint32_t tile_rank,
    uint32_t tile_world, void *d_img, void *hip_stream) {
    vk_render_params p;
    int rc = tile_call_args(scene, d_slab, d_img, width, height, output_format, tile_rank, tile_world, p);
    if (rc != VK_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return output_format == VK_OUTPUT_RGB8 ? tile_move<TM_UNPACK_U8>(d_slab, d_img, &p, TileGeom(&p), st)
                                           : tile_move<TM_UNPACK_F32>(d_slab, d_img, &p, TileGeom(&p), st);
}

int vk_to_color_device(vk_scene *scene, const void *d_rgb, uint32_t width, uint32_t height, void *d_rgb8_out, void *hip_stream) {
    if (!scene || !d_rgb || !d_rgb8_out) return fail(VK_ERR_BAD_ARG, "null argument");
    if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 31) / 3) return fail(VK_ERR_BAD_ARG, "image too large");
    HIP_TRY(hipSetDevice(scene->device));
    size_t n = (size_t)width * height * 3;
    hipLaunchKernelGGL(to_color_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       reinterpret_cast<const float *>(d_rgb), width, height, reinterpret_cast<uint8_t *>(d_rgb8_out));
    HIP_TRY(hipGetLastError());
    return VK_OK;
}

#ifdef VK_DEBUG_LIB      // libvecchio_amd_debug.so only (build.py build_device_debug): the product library holds production kernels only
// diagnostic: render with the instrumented kernel build and return the phase scheduler's counters (vecchio_amd_debug.h)
int vk_debug_phase_stats(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint64_t out[24]) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    int rc = check_render_args(scene, cam, params);
    if (rc != VK_OK) return rc;
    if (!scene->group.parts.empty() || params->output_format != VK_OUTPUT_F32) return fail(VK_ERR_UNSUPPORTED,
        "phase statistics: single device, VK_OUTPUT_F32");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(scene->device));
        int rc2 = scene->fb.ensure((size_t)params->width * params->height * 3 * sizeof(float));
        if (rc2 != VK_OK) return rc2;
        scene->want_phase_stats = true;
        rc2 = enqueue_render(scene, cam, params, scene->fb, nullptr, false, nullptr);
        scene->want_phase_stats = false;
        if (rc2 != VK_OK) return rc2;
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(out, scene->phase_stats, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return VK_OK;
    });
}

// test hook: evaluate shared-math functions on the device (host arrays in/out)
int vk_debug_math(int device, int op, const float *a, const float *b, float *out, size_t n) {
    if (!a || !b || !out) return fail(VK_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    struct DevBuf {           // freed on every exit path
        float *p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } da, db, dout;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&da.p), n * 4 + 16));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&db.p), n * 4 + 16));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dout.p), n * 4 + 16));
    HIP_TRY(hipMemcpy(da.p, a, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db.p, b, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, (const float *)da.p,
        (const float *)db.p, dout.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return VK_OK;
}

// test hook: the live device buffers, pinned buffers, events and streams of this library's handles (vk_resources.h)
int vk_debug_live_objects(uint64_t out[4]) {
    if (!out) return fail(VK_ERR_BAD_ARG, "null argument");
    for (int k = 0; k < 4; k++) out[k] = vkr::g_live[k].load();
    return VK_OK;
}

#endif

}  // extern "C"
