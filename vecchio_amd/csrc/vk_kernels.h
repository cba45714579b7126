// vk_kernels.h — the device code of libvecchio_amd.so: the persistent megakernel (render_kernel) and the small
// kernels around it (tile order, resolve, output stage, tile slabs).  Included by vk_api.hip only.
//
// Kernel structure (gfx950 / CDNA4, wave64): see the head of vk_api.hip.
#ifndef VK_KERNELS_H
#define VK_KERNELS_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/vecchio_amd.h"
#include "vk_trace.h"
#include "vk_emit.h"      // TILE, ACCUM_SCALE, to_fixed*, EmitWindow, start_camera_path: shared with vk_adapt.hip

using namespace vkd;

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;
#ifndef VK_BOX_UNROLL
#define VK_BOX_UNROLL 4
#endif
// The scheduler runs SHADE + REFILL only when its lanes outnumber the box lanes AND the primitive lanes SHADE_DEFER
// times over: a shading phase costs ~700 issue slots against ~42 of a box step, so it pays to keep traversing with
// thinning waves until nearly every lane waits for shading and then shade them all at once.  C2 / C4, Msamples/s:
// 1 (plain plurality): 4 070 / 3 435; 1.5: 4 270 / 3 645; 2: 4 430 / 3 725; 3: 4 580 / 3 815; 4: 4 630 / 3 820;
// 8: 4 600 / 3 765 (round 1).  (Deferring only against BOX, not PRIM: 4 150.)  It is a launch parameter (VK_SHADE_DEFER);
// the 1 M-sphere scene prefers the same 4 once its NaN rays no longer walk the whole tree (1 / 2 / 4 -> 573 / 588 / 593).
#ifndef VK_SHADE_DEFER
#define VK_SHADE_DEFER 4
#endif
constexpr uint32_t SHADE_DEFER = VK_SHADE_DEFER;
constexpr int BOX_UNROLL = VK_BOX_UNROLL;   // box steps between two exit tests of the BOX loop

struct KArgs {
    DScene S;
    RenderConsts C;
    float *out;              // full framebuffer (width*height*3)
    long long *accum;        // [width*height*3] fixed-point pixel sums (see to_fixed); null in the probe launch
    float4 *debug;           // optional per-sample (rgb, draws) dump
    uint32_t *counter;       // work-unit counter
    unsigned long long *clamped;   // number of samples whose radiance was clamped on its way into the fixed-point sums (see to_fixed)
    float accum_clamp;       // min(1e10, 1.3e11 / spp), worked out by the host (accum_clamp_for)
    uint32_t *launch_units;  // [2] units pulled by the 1024-thread / the other launch (the dual launch's self-check, vk_api.hip)
    uint32_t *tile_cost;     // [tiles of the image] time spent on each tile (1.6 us ticks): written by the probe (COST) build only
    const uint32_t *tile_order;   // [n_local_tiles] local tile slots, dearest first (from the probe launch), or null = raster order
    uint32_t tiles_x, tiles_y;
    uint32_t n_local_tiles;  // tiles of this call's partition
    uint32_t tile_rank, tile_world;
    uint32_t n_chunks;
    uint32_t shade_defer;    // SHADE + REFILL runs when its lanes outnumber box and primitive lanes this many times (see SHADE_DEFER)
    uint32_t prim_weight;    // pending primitive tests run when prim_weight x their lanes outnumber the box lanes
    uint32_t lds_items, lds_spheres, lds_boxes;   // record counts staged into LDS (LDS variant)
    unsigned long long *phase_stats;   // optional (diagnostic build of the kernel): 24 counters, see vk_debug_phase_stats
    // Exact re-treeing (vk_trace.h): samples dropped by the first launch (the winner of one of their segments may depend on the visiting
    // order) are queued here, REDO_REGIONS queues of redo_region_cap entries {x | y << 16, sample}, one counter per region (64 bytes
    // apart); a workgroup appends to the region of its block index.  The second launch (list_mode = 1, S = the scene as handed over)
    // takes its units from these queues instead of from the tiles: unit u = entries [n k, n (k + 1)) of region u % REDO_REGIONS,
    // k = u / REDO_REGIONS, for k below the slice count redo_plan_kernel leaves in redo_plan[0] and n = redo_plan[3] entries per unit.
    // redo_list == null: nothing is dropped
    // (the probe launch, scenes without a rebuilt tree).
    // list_mode = 2: the FALLBACK launch behind the second one — an ordinary launch over the tiles on the scene as handed over, which runs
    // only if redo_plan[2] != 0, i.e. if a queue overflowed and the frame of the first two launches is incomplete (redo_reset_kernel has
    // zeroed the sums by then); otherwise every workgroup returns at once.
    uint2 *redo_list; uint32_t *redo_count; const uint32_t *redo_plan; uint32_t redo_region_cap; uint32_t list_mode;
    // diagnostic builds (-DVK_WAVE_TIMES, with the environment's VK_WAVE_TIMES=1): per wave {start, last unit pull, end}, 100 MHz ticks
    unsigned long long *wave_times;
    // progressive rendering (vk_progress_step): this launch renders the sample WINDOW [sample_base, sample_base + C.spp) of every pixel;
    // 0 for vk_render.  A unit's samples are numbered from it, so the RNG keys (seed, pixel, sample) are those of the one-shot frame.
    uint32_t sample_base;
    // adaptive progressive rendering (vk_progress_set_adaptive): the number of active tiles, in device memory (written by the compaction
    // ahead of the launch); units are then those of the first *active_count slots of tile_order (the active list).  Null: n_local_tiles.
    const uint32_t *active_count;
};
constexpr uint32_t REDO_REGIONS = 512u;
constexpr uint32_t REDO_COUNT_STRIDE = 16u;        // uint32 words between two regions' counters
// most queue entries per work unit of the second launch (redo_plan_kernel picks 64..this)
constexpr uint32_t REDO_UNIT = 256u;

// LDS-resident hot records
struct LdsMem {
    const uint4 *items;      // first halves of all items (x/y bounds) ...
    const uint4 *items_hi;   // ... then the second halves (z bounds, w0, w1): 16-byte stride per array gives a
                             // ds_read_b128 16 bank slots instead of the 8 a 32-byte stride leaves it
    const float4 *spheres;
    const uint4 *boxes;      // 2 x uint4 per DBox
    const uint32_t *sphere_mat;
    __device__ __forceinline__ DBox box(uint32_t i) const {
        uint4 a = boxes[2 * i], b = boxes[2 * i + 1];
        DBox o;
        o.p0[0] = __uint_as_float(a.x); o.p0[1] = __uint_as_float(a.y); o.p0[2] = __uint_as_float(a.z);
        o.p1x = __uint_as_float(a.w); o.p1y = __uint_as_float(b.x); o.p1z = __uint_as_float(b.y);
        o.mat = b.z; o._p = 0;
        return o;
    }
    // the traversal cursor counts BYTES of these two arrays (16 per item; see GlobalMem::ISHIFT): the skip links of the staged
    // items are scaled to match when a workgroup copies them in (render_kernel)
    static constexpr uint32_t ISHIFT = 4;
    static constexpr bool FUSED_BOX = true;      // see GlobalMem
    uint32_t items_hi_off;   // byte offset of items_hi in the workgroup's LDS
    __device__ __forceinline__ DItem item(uint32_t off) const {
        // Absolute LDS addresses: the staged scene starts at LDS address 0 (the kernels have no static LDS: pinned by
        // tests/test_kernel_resources.py), so the cursor IS the address of the first half.  Through `smem` the compiler adds
        // the array's link-time address (0) with a VALU instruction per read.
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        typedef const u32x4 __attribute__((address_space(3))) *lds_u4;
        u32x4 a = *(lds_u4)(uintptr_t)off;
        u32x4 b = *(lds_u4)(uintptr_t)(off + items_hi_off);
        DItem n;
        n.mnx = __uint_as_float(a.x); n.mxx = __uint_as_float(a.y); n.mny = __uint_as_float(a.z); n.mxy = __uint_as_float(a.w);
        n.mnz = __uint_as_float(b.x); n.mxz = __uint_as_float(b.y);
        n.w0 = b.z; n.w1 = b.w;
        return n;
    }
    __device__ __forceinline__ DSphere sphere(uint32_t i) const {
        float4 s = spheres[i];
        DSphere o; o.cx = s.x; o.cy = s.y; o.cz = s.z; o.r = s.w;
        return o;
    }
    __device__ __forceinline__ uint32_t smat(uint32_t i) const { return sphere_mat[i]; }
    // the grid form (DGrid): the staged table [cells | refs] takes the items' place at LDS address 0
    __device__ __forceinline__ uint32_t grid_cell(const DScene &, uint32_t c) const {
        typedef const uint32_t __attribute__((address_space(3))) *lds_u;
        return *(lds_u)(uintptr_t)(c << 2);
    }
    __device__ __forceinline__ uint32_t grid_ref(const DScene &S, uint32_t k) const {
        typedef const uint32_t __attribute__((address_space(3))) *lds_u;
        return *(lds_u)(uintptr_t)((S.grid.nu * S.grid.nv + 1u + k) << 2);
    }
};

extern __shared__ uint4 smem[];

// The persistent loop below is one big region; left alone, LLVM hoists every value that is
// invariant across it (seed hashes, camera terms, scene pointers, division magic numbers)
// into the prologue and then spills them (>1 KB of scratch per lane, reloaded inside the hot
// loop).  So nothing is read from the by-value kernel argument directly: each phase re-reads
// what it needs from the kernarg segment (scalar loads, K$-resident) through a pointer that
// is laundered by an empty asm, which pins the loads, and everything derived from them,
// inside the phase that uses them.
typedef const __attribute__((address_space(4))) KArgs *KArgsC;
__device__ __forceinline__ KArgsC kargs_fresh() {
    KArgsC p = (KArgsC)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#define KARG(p, field) (*(const decltype(KArgs::field) *)&((p)->field))

template <uint32_t F, bool LDS_SCENE>
__device__ __forceinline__ typename std::conditional<LDS_SCENE, LdsMem, GlobalMem>::type make_mem(const DScene &S, uint32_t lds_items) {
    typename std::conditional<LDS_SCENE, LdsMem, GlobalMem>::type M;
    if constexpr (LDS_SCENE) {
        M.items = smem; M.items_hi = smem + lds_items; M.items_hi_off = lds_items << 4;
        M.spheres = reinterpret_cast<const float4 *>(smem + 2u * lds_items);
        M.boxes = smem + 2u * lds_items + S.n_spheres; M.sphere_mat = S.sphere_mat;
    } else {
        M.items = S.items; M.spheres = S.spheres; M.sphere_mat = S.sphere_mat; M.boxes = S.boxes;
    }
    return M;
}

// Cold per-lane path state lives in LDS between SHADE phases, SoA by field (word f of lane l at cold[f*64 + l]:
// conflict-free), so that the box/primitive loops keep only the traversal state in VGPRs: throughput (3), depth, RNG key (2)
// + counter, the sample's pixel (x | y << 16) and sample index (+ the world-space ray (o3 d3) for scenes with instances).
// Radiance is not kept: no material both emits and scatters (material.rs:30-40,215-225), so it is 0 — or its NaN is implied
// by a non-finite throughput — until the path ends.
enum : int { CF_THR = 0, CF_DEPTH = 3, CF_KEY = 4, CF_CTR = 6, CF_XY = 7, CF_SAMPLE = 8, CF_WORLD_RAY = 9 };
constexpr int NCOLD_BASE = 9;
constexpr int NCOLD_INST = 15;
template <uint32_t F> constexpr int ncold() { return (F & VKF_INSTANCE) ? NCOLD_INST : NCOLD_BASE; }
constexpr int WAVE_STATE_WORDS = 8;   // per-wave, wave-uniform: the unit whose samples are being handed out (see render_kernel)
// one 16-byte record: tile origin (x | y << 16), first sample, items, items handed out
enum : int { WS_TXY = 0, WS_S0 = 1, WS_TOTAL = 2, WS_NEXT = 3,
              WS_KARGS = 4 };  // + the kernel-argument segment's address (2 words), for code that is called (shade_refill_call)

// per-wave LDS block, contiguous: [cold lane state][tile sums: 64 x 3 x u64][wave state]
template <uint32_t F> constexpr uint32_t wave_block_floats() { return 64u * (uint32_t)ncold<F>() + 64u * 3u * 2u +
    (uint32_t)WAVE_STATE_WORDS; }

// Pixel sums are ORDER-INDEPENDENT: every finished sample is added to its pixel's three 64-bit fixed-point accumulators
// (2^-26 units: 1.5e-8 absolute per sample, sums up to 1.4e11) with integer atomics, so the image does not depend on which
// lane, wave, work unit, tile partition or GPU traced a sample, nor on the order they finished in — without any lane ever
// waiting for another one's path.  (The reference's `c += color` in f32, main.rs:193, is re-associated anyway: it never
// feeds control flow.)  The sums SATURATE instead of wrapping: a sample's components are clamped to +-min(1e10, 1.3e11 / spp), so
// that spp of them stay below 2^63 * 2^-26 = 1.37e11, and every clamped sample is counted (vk_stats.clamped_samples): the reference
// adds such a sample in f32 (main.rs:193) and the caller can tell that this frame deviates from it.  (ACCUM_SCALE, to_fixed_small and
// to_fixed: vk_emit.h)
constexpr float ACCUM_CLAMP = 1.0e10f;
constexpr float ACCUM_RANGE = 1.3e11f;
inline float accum_clamp_for(uint32_t spp) { float c = ACCUM_RANGE / (float)spp; return c < ACCUM_CLAMP ? c : ACCUM_CLAMP; }     // (host)
// (ACCUM_SMALL, the bound of to_fixed_small's operand: vk_emit.h)

template <uint32_t F>
__device__ __forceinline__ void cold_store_path(float *c, uint32_t lane, const Lane &L) {
    c[(CF_THR + 0) * 64 + lane] = L.thr.x; c[(CF_THR + 1) * 64 + lane] = L.thr.y; c[(CF_THR + 2) * 64 + lane] = L.thr.z;
    c[CF_DEPTH * 64 + lane] = __uint_as_float(L.depth);
    c[CF_KEY * 64 + lane] = __uint_as_float((uint32_t)L.rng.key);
    c[(CF_KEY + 1) * 64 + lane] = __uint_as_float((uint32_t)(L.rng.key >> 32));
    c[CF_CTR * 64 + lane] = __uint_as_float(L.rng.ctr);
    if (F & VKF_INSTANCE) {
        c[(CF_WORLD_RAY + 0) * 64 + lane] = L.wo.x; c[(CF_WORLD_RAY + 1) * 64 + lane] = L.wo.y; c[(CF_WORLD_RAY + 2) * 64 + lane] = L.wo.z;
        c[(CF_WORLD_RAY + 3) * 64 + lane] = L.wd.x; c[(CF_WORLD_RAY + 4) * 64 + lane] = L.wd.y; c[(CF_WORLD_RAY + 5) * 64 + lane] = L.wd.z;
    }
}
template <uint32_t F>
__device__ __forceinline__ void cold_load_world_ray(const float *c, uint32_t lane, Lane &L) {
    if (F & VKF_INSTANCE) {
        L.wo = v3(c[(CF_WORLD_RAY + 0) * 64 + lane], c[(CF_WORLD_RAY + 1) * 64 + lane], c[(CF_WORLD_RAY + 2) * 64 + lane]);
        L.wd = v3(c[(CF_WORLD_RAY + 3) * 64 + lane], c[(CF_WORLD_RAY + 4) * 64 + lane], c[(CF_WORLD_RAY + 5) * 64 + lane]);
    }
}
template <uint32_t F>
__device__ __forceinline__ void cold_load_path(const float *c, uint32_t lane, Lane &L) {
    L.thr = v3(c[(CF_THR + 0) * 64 + lane], c[(CF_THR + 1) * 64 + lane], c[(CF_THR + 2) * 64 + lane]);
    L.acc = v3s(0.0f);
    L.depth = __float_as_uint(c[CF_DEPTH * 64 + lane]) & 0x7FFFFFFFu;      // (bit 31: shade_refill_body's rearm mark)
    L.rng.key = (uint64_t)__float_as_uint(c[CF_KEY * 64 + lane]) | ((uint64_t)__float_as_uint(c[(CF_KEY + 1) * 64 + lane]) << 32);
    L.rng.ctr = __float_as_uint(c[CF_CTR * 64 + lane]);
    L.pixel = 0; L.sample = 0;
    if (F & VKF_INSTANCE) cold_load_world_ray<F>(c, lane, L);
    else { L.wo = L.o; L.wd = L.d; }       // no instances: the current space IS world space
}

// adds the wave's LDS sums of tile `txy` (x | y << 16 of its origin; lane = pixel slot) to the frame's accumulators and clears them
__device__ __forceinline__ void flush_tile_sums(unsigned long long *tile_sum, long long *accum, uint32_t txy, uint32_t lane,
    uint32_t width, uint32_t height) {
    uint32_t px = (txy & 0xFFFFu) + (lane & 7u), py = (txy >> 16) + (lane >> 3);
    if (!accum || txy == 0xFFFFFFFFu || px >= width || py >= height) return;
    unsigned long long *a = reinterpret_cast<unsigned long long *>(accum) + ((size_t)py * width + px) * 3;
    for (int c = 0; c < 3; c++) {
        unsigned long long v = tile_sum[lane * 3 + c];
        if (v) { atomicAdd(a + c, v); tile_sum[lane * 3 + c] = 0ull; }
    }
}

// number of lanes of the wave for which p holds (v_cmp -> s_bcnt1, no VGPR round trip)
// lane mask of prim_is_heavy<F>(ref), straight from the compare
template <uint32_t F>
__device__ __forceinline__ unsigned long long heavy_mask(uint32_t ref) {
    if constexpr ((F & VKF_ALL_SCENE) == VKF_ALL_SCENE) return __builtin_amdgcn_uicmp(ref - ((uint32_t)DK_LIST << 28), 3u << 28,
        36 /* ult */);
    else return __builtin_amdgcn_uicmp(ref, (uint32_t)DK_LIST << 28, 35 /* uge */);
}
__device__ __forceinline__ uint32_t lanes_with(bool p) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }

// ---- Perlin turbulence, the octaves of one lane spread over the wave.  perlin_turb is seven octaves of an 8-corner noise (56
// dependent gathers) and, in a scene like the final one, is needed by one or two of a shading phase's 64 lanes in three phases out of
// four: run inside the material code it keeps the whole wave for seven serial noise evaluations.  The octaves are independent until
// the final ordered sum, so here — at a point of the phase where every lane of the wave is present — the lanes that WILL evaluate a
// noise texture are found ahead of the material code (a sphere hit outside any instance: its point is o + d*T; the lineariser lists
// the few spheres with a noise material) and, nine of them per round, 63 helper lanes each evaluate one octave of one of them; points
// and values travel by ds_bpermute and each served lane sums its seven values in the reference's order (accum += weight * noise,
// material.rs:379-390: scaling the point and the weight by powers of two is exact, so octave j alone computes what iteration j of the
// loop does).  texture_value uses the value only for the texture and point it was made for and runs the loop itself otherwise (lists,
// instanced objects, SpecDiffuse picks).  C3: 763 -> 799 Msamples/s (with ONE octave instead of seven, i.e. no turbulence cost left
// to remove, it would be 809).
template <uint32_t F, class Mem>
__device__ __forceinline__ PreTurb cooperative_turb(const Lane &L, const DScene &S, const Mem &M, bool is_shade, uint32_t lane) {
    PreTurb pt = no_pre_turb();
    if constexpr ((F & VKF_TEXTURES) != 0u) {
        if (!(S.features & VKF_NOISE)) return pt;          // (wave-uniform) no noise texture in this scene: nothing to prepare
        uint32_t perlin = 0u;
        if (is_shade && L.best_prim != 0u && VKD_KIND(L.best_prim) == DK_SPHERE && (!(F & VKF_INSTANCE) || L.best_inst < 0)) {
            const uint32_t idx = VKD_INDEX(L.best_prim);
            if (S.n_noise_spheres != 0xFFFFFFFFu) {        // the scene's (few) spheres with a noise material, from the lineariser
                for (uint32_t k = 0; k < 4u; k++)
                    if (k < S.n_noise_spheres && idx == S.noise_sphere[k]) { pt.tex = S.noise_tex[k]; perlin = S.noise_perlin[k]; }
            } else {
                const DMaterial &m = S.materials[M.smat(idx)];
                if (m.tex_kind == VK_TEX_NOISE) { pt.tex = m.tex; perlin = S.textures[m.tex].a; }
            }
            if (pt.tex != 0xFFFFFFFFu) {
                V3 p = L.o + L.d * L.T;                    // simple_record's R.p for a sphere
                pt.px = p.x; pt.py = p.y; pt.pz = p.z;
            }
        }
        unsigned long long todo = __builtin_amdgcn_uicmp(pt.tex, 0xFFFFFFFFu, 33 /* ne */);
        if (todo != 0ull) {                                // wave-uniform: every lane of the wave is here
            // Up to nine lanes' turbulences per round: helper lane h < 63 evaluates octave h % 7 for the (h / 7)-th of them, so that
            // the noise evaluation — two dependent rounds of gathers — is paid once per round, not once per lane that needs one
            const uint32_t my_rank = (uint32_t)__builtin_popcountll(todo & ((1ull << lane) - 1ull));   // of a lane that needs one
            const uint32_t my_slot = lane / 7u, my_octave = lane - 7u * my_slot;
            uint32_t base = 0u;
            while (todo != 0ull) {
                uint32_t my_src = 0u; bool helper = false;
                for (uint32_t sl = 0; sl < 9u; sl++) {
                    if (todo == 0ull) break;               // (uniform)
                    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    if (my_slot == sl) { my_src = src; helper = true; }
                }
                const int sa = (int)(my_src << 2);
                const float sx = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(sa, (int)__float_as_uint(pt.px)));
                const float sy = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(sa, (int)__float_as_uint(pt.py)));
                const float sz = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(sa, (int)__float_as_uint(pt.pz)));
                const uint32_t sp = (uint32_t)__builtin_amdgcn_ds_bpermute(sa, (int)perlin);
                float n = 0.0f;
                if (helper) {
                    const float sc = (float)(1u << my_octave); // the point of this octave: p * 2^octave, exactly what the doublings give
                    n = perlin_noise(S.perlins[sp], v3(sx * sc, sy * sc, sz * sc));
                }
                // the lanes served this round sum their seven values in the reference's order
                const uint32_t slot = my_rank - base;      // (meaningful for lanes with a pending request of this round only)
                float accum = 0.0f, weight = 1.0f;
                for (uint32_t j = 0; j < 7u; j++) {
                    const int ga = (int)(((slot < 9u ? slot : 0u) * 7u + j) << 2);
                    accum += weight * __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(ga, (int)__float_as_uint(n)));
                    weight *= 0.5f;
                }
                // (my_rank >= base for lanes not served yet; < base wraps to huge)
                if (pt.tex != 0xFFFFFFFFu && slot < 9u) pt.val = fabsf(accum);
                base += 9u;
            }
        }
    }
    return pt;
}

// ---- random_in_unit_sphere for the lanes about to scatter off a Metal (or an Isotropic), drawn by the WHOLE wave.  The rejection loop
// (util.rs:31-40) accepts 52 % of its candidates: run lane by lane, a wave with ten such lanes iterates four times on average, and
// removing the loop altogether would make the InOneWeekend scene 7.7 % faster (profiles/r05/experiments).  The generator is
// counter-based — candidate m of a lane's loop is draws ctr + 3m + 1 .. 3 of its stream, whoever computes them — so the 64 lanes are
// dealt evenly to the K lanes that need a point: lane h draws candidate h mod G of the lane of rank h / G, G = 64 / K, and the
// owner takes the first one inside the sphere (the loop's own choice).  One round nearly always does (0.476^6 = 1 %); the rest go round
// again with the wave regrouped.
__device__ __forceinline__ PreBall cooperative_ball(bool want, const Rng &rng, uint32_t lane) {
    PreBall out = no_pre_ball();
    uint32_t m0 = 0u;                                    // candidates of this lane's loop already refused
    unsigned long long need = __builtin_amdgcn_ballot_w64(want);
    while (need != 0ull) {                               // (wave-uniform)
        const uint32_t K = (uint32_t)__popcll(need), G = 64u / K;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        // table rank -> lane (a push: lanes that need nothing write entry 63, which is an owner's only when all 64 are)
        const int tbl = __builtin_amdgcn_ds_permute((int)((want ? rank : 63u) << 2), (int)lane);
        const uint32_t j = (lane * ((65536u + G - 1u) / G)) >> 16;      // lane / G (exact below 64)
        const uint32_t c = lane - j * G;
        const int owner = __builtin_amdgcn_ds_bpermute((int)((j < 63u ? j : 63u) << 2), tbl) << 2;
        const uint32_t klo = (uint32_t)__builtin_amdgcn_ds_bpermute(owner, (int)(uint32_t)rng.key);
        const uint32_t khi = (uint32_t)__builtin_amdgcn_ds_bpermute(owner, (int)(uint32_t)(rng.key >> 32));
        const uint32_t cb = (uint32_t)__builtin_amdgcn_ds_bpermute(owner, (int)(rng.ctr + 3u * m0));
        bool inside;
        const V3 p = ball_candidate((uint64_t)klo | ((uint64_t)khi << 32), cb + 3u * c, inside);
        const unsigned long long fl = __builtin_amdgcn_ballot_w64(inside && j < K);
        // the owner's helpers are lanes rank * G .. rank * G + G - 1
        const uint32_t lo = rank * G;
        const unsigned long long grp = want ? ((fl >> (lo & 63u)) & (G == 64u ? ~0ull : ((1ull << G) - 1ull))) : 0ull;
        const uint32_t first = grp ? (uint32_t)__builtin_ctzll(grp) : 0u;
        const int src = (int)(((lo + first) & 63u) << 2);
        const float x = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)__float_as_uint(p.x)));
        const float y = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)__float_as_uint(p.y)));
        const float z = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)__float_as_uint(p.z)));
        if (want) {
            if (grp) { want = false; out.have = 1u; out.p = v3(x, y, z); out.skip = 3u * (m0 + first + 1u); }
            else m0 += G;
        }
        need = __builtin_amdgcn_ballot_w64(want);
    }
    return out;
}

// ---- the SHADE + REFILL phase body: shade the lanes whose segment is fully traversed, deposit finished samples, hand new
// samples to the lanes without a path.  Leaves `fresh` lanes with a new ray parked in L.wo / L.wd / L.time, which the caller
// installs with ONE begin_segment (its three exact reciprocals are ~60 instructions per call site). Used inline by the lean variants and
// through shade_refill_call (below) by the everything-variants.
struct PhaseClocks { unsigned long long mat = 0, refill = 0, t1 = 0, turb = 0, cold = 0; };
template <uint32_t F, bool LDS_SCENE, bool STATS, bool COST>
__device__ __forceinline__ void shade_refill_body(Lane &L, bool is_shade, bool early, bool &active, bool &need, bool &fresh, bool &touched,
                                                  bool &rearm,
                                                  uint32_t &cost_t0, KArgsC P, float *cold, unsigned long long *tile_sum,
                                                  uint32_t *wstate, uint32_t lane, uint32_t lds_items, PhaseClocks &clk) {
    using Mem = typename std::conditional<LDS_SCENE, LdsMem, GlobalMem>::type;
    RenderConsts C = KARG(P, C);
    DScene S = KARG(P, S);
    Mem M = make_mem<F, LDS_SCENE>(S, lds_items);
    unsigned long long &st_t_mat = clk.mat, &st_t_refill = clk.refill, &st_t1 = clk.t1;
    (void)st_t_mat; (void)st_t_refill; (void)st_t1; (void)cost_t0;
    fresh = false;                // lanes that leave this phase with a new ray to install; it is parked in the
                                  // (dead) world-ray fields L.wo / L.wd / L.time, so it costs no registers
    if (STATS) st_t1 = clock64();
    const PreTurb pre_turb = cooperative_turb<F, Mem>(L, S, M, is_shade, lane);
    if (STATS) clk.turb += clock64() - st_t1;
    rearm = false;
    // `early` (exact re-treeing): the winner of this lane's segment may depend on the visiting order (vk_trace.h segment_unsafe,
    // asked by the caller, which holds the segment's reciprocals)
    if constexpr ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u && !LDS_SCENE) {
        // scene in global memory (both trees in items[], DScene::walk_start): the segment is walked again, now on the tree as handed
        // over — the caller re-installs the same ray for that; bit 31 of the lane's depth word says so until the segment is shaded
        if (S.walk_start != 0u && is_shade && early) {
            rearm = true; is_shade = false;
            L.wo = L.o; L.wd = L.d;      // (L.time is the segment's)
            cold[CF_DEPTH * 64 + lane] = __uint_as_float(__float_as_uint(cold[CF_DEPTH * 64 + lane]) | 0x80000000u);
        }
    }
    if constexpr ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) {
        // scene in LDS (the rebuilt tree only) — and the grid form wherever it is walked from: the sample of such a segment is dropped
        // here (a queue was handed in: redo_list) and rendered by the second launch on the
        // tree as handed over.  One counter update per wave and phase, prefix sums over the dropping lanes.
        uint2 *rl = KARG(P, redo_list);
        const unsigned long long m_drop = __builtin_amdgcn_ballot_w64(is_shade && early && rl != nullptr);
        if (m_drop != 0ull) {
            // (dual launch: 0..255 | 256..511)
            const uint32_t region = (blockIdx.x + (blockDim.x == 1024u ? 0u : gridDim.x)) & (REDO_REGIONS - 1u);
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(KARG(P, redo_count) + region * REDO_COUNT_STRIDE, (uint32_t)__popcll(m_drop));
            base = __builtin_amdgcn_readfirstlane(base);
            if ((m_drop >> lane) & 1ull) {
                const uint32_t slot = base + (uint32_t)__popcll(m_drop & ((1ull << lane) - 1ull));
                const uint32_t cap = KARG(P, redo_region_cap);
                // (a full region: the counter keeps counting and the host sees the overflow, vk_api.hip)
                if (slot < cap) rl[(size_t)region * cap + slot] = make_uint2(__float_as_uint(cold[CF_XY * 64 + lane]),
                    __float_as_uint(cold[CF_SAMPLE * 64 + lane]));
                is_shade = false; active = false; need = true;
            }
        }
    }
    touched = is_shade;
    PreBall pre_ball = no_pre_ball();
    if constexpr (F == 0u && LDS_SCENE) {
        // (the sphere-only scatter variant staged in LDS — the headline's: the material is one gather away, shade_core reads the same
        // record; before the path's other cold state is loaded: the traversal state of the lanes that are not shading stays live
        // through this phase, registers are short.  Its PDF twin and the global-memory variants would spill more than they gain.)
        bool want = false;
        Rng g; g.key = 0ull; g.ctr = 0u;
        if (is_shade && L.best_prim != 0u) {
            const uint32_t kind = S.sphere_material[VKD_INDEX(L.best_prim)].kind;
            want = kind == VK_MAT_METAL || kind == VK_MAT_ISOTROPIC;
        }
        if (want) {
            g.key = (uint64_t)__float_as_uint(cold[CF_KEY * 64 + lane]) | ((uint64_t)__float_as_uint(cold[(CF_KEY + 1) * 64 + lane]) << 32);
            g.ctr = __float_as_uint(cold[CF_CTR * 64 + lane]);
        }
        pre_ball = cooperative_ball(want, g, lane);
    }
    if (is_shade) {
        if (STATS) st_t1 = clock64();
        cold_load_path<F>(cold, lane, L);
        if (STATS) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); clk.cold += clock64() - st_t1; }
    }
    if (is_shade) {
        if (STATS) st_t1 = clock64();
        V3 no, nd; float nt;
        bool cont = shade_core<F, Mem>(L, S, M, C, no, nd, nt, pre_turb, pre_ball);
        if (cont) { L.wo = no; L.wd = nd; L.time = nt; fresh = true; }
        if (STATS) st_t_mat += clock64() - st_t1;
        if (!cont) {
            uint32_t xy = __float_as_uint(cold[CF_XY * 64 + lane]);
            size_t pix = (size_t)(xy >> 16) * C.width + (xy & 0xFFFFu);
            float4 *dbg = KARG(P, debug);
            if (dbg) dbg[pix * C.spp + (__float_as_uint(cold[CF_SAMPLE * 64 + lane]) - KARG(P, sample_base))] = make_float4(L.acc.x, L.acc.y, L.acc.z,
                __uint_as_float(L.rng.ctr));
            long long *acc = KARG(P, accum);
            if (acc && isfinite(L.acc.x) && isfinite(L.acc.y) && isfinite(L.acc.z)) {   // main.rs:192-194; c += color (main.rs:193)
                const float clampv = KARG(P, accum_clamp);
                const float big = fmaxf(fmaxf(fabsf(L.acc.x), fabsf(L.acc.y)), fabsf(L.acc.z));
                unsigned long long fx, fy, fz;
                if (big <= ACCUM_SMALL) {      // (nearly always, for the whole wave)
                    fx = (unsigned long long)to_fixed_small(L.acc.x); fy = (unsigned long long)to_fixed_small(L.acc.y);
                    fz = (unsigned long long)to_fixed_small(L.acc.z);
                } else {
                    if (big > clampv) atomicAdd(KARG(P, clamped), 1ull);     // (rare)
                    fx = (unsigned long long)to_fixed(L.acc.x, clampv); fy = (unsigned long long)to_fixed(L.acc.y, clampv);
                    fz = (unsigned long long)to_fixed(L.acc.z, clampv);
                }
                // a sample of the tile the wave is handing out (nearly all of them) lands in the wave's LDS sums, which
                // reach the frame's accumulators once per unit; a straggler of an earlier unit goes there directly
                if ((xy & 0xFFF8FFF8u) == __builtin_amdgcn_readfirstlane(wstate[WS_TXY])) {
                    unsigned long long *t = tile_sum + ((xy & 7u) | ((xy >> 13) & 0x38u)) * 3u;
                    atomicAdd(t + 0, fx); atomicAdd(t + 1, fy); atomicAdd(t + 2, fz);
                } else {
                    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc) + pix * 3;
                    atomicAdd(a + 0, fx); atomicAdd(a + 1, fy); atomicAdd(a + 2, fz);
                }
            }
            if (COST) {   // probe launch: the lane-time this sample took, charged to its tile
                uint32_t *tc = KARG(P, tile_cost);
                uint32_t now = (uint32_t)(wall_clock64() >> 4);
                if (tc) atomicAdd(&tc[((xy >> 16) / TILE) * KARG(P, tiles_x) + (xy & 0xFFFFu) / TILE], now - cost_t0);
            }
            active = false;
            need = true;
        }
    }
    if (STATS) st_t1 = clock64();
    // ---- hand out samples of the wave's current unit to the lanes without a path; pull the next unit when it is used up
    for (;;) {
        unsigned long long need_mask = __builtin_amdgcn_ballot_w64(need);
        if (!need_mask) break;
        uint4 ws = *reinterpret_cast<const uint4 *>(wstate);       // one ds_read_b128, the same address in every lane
        uint32_t txy = __builtin_amdgcn_readfirstlane(ws.x), s0 = __builtin_amdgcn_readfirstlane(ws.y);
        uint32_t total = __builtin_amdgcn_readfirstlane(ws.z), next = __builtin_amdgcn_readfirstlane(ws.w);
        // the second launch of exact re-treeing (sphere-only variants): units are slices of the redo queues
        const bool list_mode = ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) && KARG(P, list_mode) == 1u;
        if (next >= total) {
            uint32_t unit = 0;
            if (lane == 0) {
                unit = atomicAdd(KARG(P, counter), 1u);
                // (once per 2 048 samples or more; the dual launch's self-check counts the first launch's units only)
                if (KARG(P, list_mode) == 0u) atomicAdd(KARG(P, launch_units) + (blockDim.x == 1024u ? 0 : 1), 1u);
            }
            unit = __builtin_amdgcn_readfirstlane(unit);
            if (list_mode) {
                const uint32_t cap = KARG(P, redo_region_cap);
                const uint32_t *plan = KARG(P, redo_plan);
                const uint32_t usize = plan[3];                 // entries per unit (redo_plan_kernel)
                if (unit >= REDO_REGIONS * plan[0]) { need = false; break; }
                flush_tile_sums(tile_sum, KARG(P, accum), txy, lane, C.width, C.height);      // (nothing after the first unit)
                const uint32_t region = unit % REDO_REGIONS, first = (unit / REDO_REGIONS) * usize;
                uint32_t cnt = KARG(P, redo_count)[region * REDO_COUNT_STRIDE];
                cnt = __builtin_amdgcn_readfirstlane(cnt < cap ? cnt : cap);
                txy = 0xFFFFFFFEu;                              // no tile: every sample goes to the frame's sums directly
                s0 = region * cap + first;                      // (here: the unit's first queue entry)
                next = 0u; total = first < cnt ? (cnt - first < usize ? cnt - first : usize) : 0u;
                if (lane == 0) { wstate[WS_TXY] = txy; wstate[WS_S0] = s0; wstate[WS_TOTAL] = total; wstate[WS_NEXT] = 0u; }
                if (total == 0u) continue;                      // an empty slice: the next unit
            } else {
            const uint32_t n_chunks = KARG(P, n_chunks);
#ifdef VK_WAVE_TIMES
            { unsigned long long *wt = KARG(P, wave_times);
              if (wt && lane == 0) wt[3u * ((blockIdx.x + (blockDim.x == 1024u ? 0u : gridDim.x)) * 16u + (threadIdx.x >> 6)) + 1u] = wall_clock64(); }
#endif
            // adaptive windows: the units of the active tiles only (a uniform load, once per unit pull)
            const uint32_t *ac = KARG(P, active_count);
            const uint32_t n_tiles = ac ? __builtin_amdgcn_readfirstlane(*ac) : KARG(P, n_local_tiles);
            if (unit >= n_tiles * n_chunks) {                                     // the launch's units are all handed out:
                need = false;                                                     // these lanes idle until the wave's last path ends
                break;
            }
            flush_tile_sums(tile_sum, KARG(P, accum), txy, lane, C.width, C.height);  // the finished unit's sums so far
            const uint32_t chunk = unit % n_chunks;
            // tiles are visited dearest-first when the probe launch left an order (see enqueue_render)
            uint32_t tslot = unit / n_chunks;
            { const uint32_t *ord = KARG(P, tile_order); if (ord) tslot = ord[tslot]; }
            const uint32_t tile = KARG(P, tile_rank) + tslot * KARG(P, tile_world);
            const uint32_t tiles_x = KARG(P, tiles_x);
            s0 = (uint32_t)(((uint64_t)C.spp * chunk) / n_chunks);
            const uint32_t s1 = (uint32_t)(((uint64_t)C.spp * (chunk + 1)) / n_chunks);
            txy = ((tile % tiles_x) * TILE) | (((tile / tiles_x) * TILE) << 16);
            next = 0u; total = 64u * (s1 - s0);
            s0 += KARG(P, sample_base);                                           // the window's first sample (0: vk_render)
            if (lane == 0) { wstate[WS_TXY] = txy; wstate[WS_S0] = s0; wstate[WS_TOTAL] = total; }
            }
        }
        uint32_t k = next + (uint32_t)__popcll(need_mask & ((1ull << lane) - 1ull));
        if (need && k < total) {
            uint32_t q = k & 63u, smp = s0 + (k >> 6);
            uint32_t px = (txy & 0xFFFFu) + (q & 7u), py = (txy >> 16) + (q >> 3);
            if (list_mode) {
                const uint2 e = KARG(P, redo_list)[(size_t)s0 + k];
                px = e.x & 0xFFFFu; py = e.x >> 16; smp = e.y;
            }
            if (px < C.width && py < C.height) {   // slots outside the image (edge tiles) are skipped: the lane asks again
                cold[CF_XY * 64 + lane] = __uint_as_float(px | (py << 16));
                cold[CF_SAMPLE * 64 + lane] = __uint_as_float(smp);
                if (COST) cost_t0 = (uint32_t)(wall_clock64() >> 4);
                V3 no, nd; float nt;               // the lane's next sample (main.rs:186-190)
                start_sample_core(L, C, px, py, smp, no, nd, nt);
                L.wo = no; L.wd = nd; L.time = nt;
                fresh = true;
                active = true;
                need = false;
                touched = true;
            }
        }
        uint32_t taken = (uint32_t)__popcll(need_mask);
        if (lane == 0) wstate[WS_NEXT] = next + taken < total ? next + taken : total;
    }
    if (STATS) { st_t_refill += clock64() - st_t1; st_t1 = clock64(); }
}

// The everything-variants (media + textures + instances + lists) call the phase out of line: its several hundred live
// values then get their own register allocation instead of squeezing the traversal loops' (left inline, the allocator spilled
// traversal state inside the box and primitive loops as soon as anything in the kernel changed: C3 moved between 330 and 520
// Msamples/s with the spill placement).  Only what shading reads of the traversal state crosses, by value.
struct ShadeIo {
    // in: 1 is_shade, 2 active, 4 need, 64 early (segment_unsafe);   out: 2 active, 4 need, 8 fresh, 16 touched, 32 rearm (same ray
    // again)
    uint32_t flags;
    float T; uint32_t best_prim; int32_t best_inst; float best_aux;
    V3 o, d; float time;       // in: the segment's ray (world ray when the scene has no instances); out: the new ray of fresh lanes
    uint32_t cost_t0;
};
template <uint32_t F, bool LDS_SCENE, bool COST>
__device__ __attribute__((noinline)) ShadeIo shade_refill_call(ShadeIo io, uint32_t lds_items, uint32_t wave_block) {
    // a called function has neither the kernel-argument pointer nor the kernel's LDS pointers: the wave's LDS block comes as its
    // offset in the workgroup's dynamic LDS, and the kernel left the argument segment's address in the wave state
    const uint32_t lane = threadIdx.x & 63u;
    float *cold = reinterpret_cast<float *>(smem) + wave_block;
    unsigned long long *tile_sum = reinterpret_cast<unsigned long long *>(cold + 64 * ncold<F>());
    uint32_t *wstate = reinterpret_cast<uint32_t *>(cold + 64 * ncold<F>() + 64 * 3 * 2);
    KArgsC P;
    {
        uint64_t a = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(wstate[WS_KARGS]) |
                     ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(wstate[WS_KARGS + 1]) << 32);
        P = (KArgsC)a;
        asm volatile("" : "+s"(P));
    }
    Lane L;
    __builtin_memset(&L, 0, sizeof(L));     // (the intrinsic: HIP's device memset() is a loop, which keeps a Lane this large in scratch)
    L.T = io.T; L.best_prim = io.best_prim; L.best_inst = io.best_inst; L.best_aux = io.best_aux;
    L.o = io.o; L.d = io.d; L.time = io.time;
    bool active = (io.flags & 2u) != 0u, need = (io.flags & 4u) != 0u, fresh = false, touched = false, rearm = false;
    uint32_t cost_t0 = io.cost_t0;
    PhaseClocks clk;
    shade_refill_body<F, LDS_SCENE, false, COST>(L, (io.flags & 1u) != 0u, (io.flags & 64u) != 0u, active, need, fresh, touched, rearm,
        cost_t0, P, cold, tile_sum,
        wstate, lane, lds_items, clk);
    // fresh lanes: L.wo / L.wd hold the NEW ray, which is what the world-ray slots want
    if (active && touched) cold_store_path<F>(cold, lane, L);
    ShadeIo out = io;
    out.flags = (active ? 2u : 0u) | (need ? 4u : 0u) | (fresh ? 8u : 0u) | (touched ? 16u : 0u) | (rearm ? 32u : 0u);
    out.o = L.wo; out.d = L.wd; out.time = L.time; out.cost_t0 = cost_t0;
    return out;
}

// Work distribution.  A work UNIT is (8x8 tile, sample chunk), pulled by a WAVE from a global atomic counter and handed
// out to its lanes sample by sample (item k -> pixel slot k & 63, sample s0 + (k >> 6): the 64 primary rays of one sample
// index start together, which keeps the first segments coherent).  A lane whose path ended takes the next item by ballot +
// prefix popcount (active-ray compaction), and the wave pulls the NEXT unit the moment the current one is handed out:
// nobody waits for the slowest path of a unit (the "drain" cost 5 % on C2 and most of the lanes on C5). That is possible because pixel sums
// are order independent (to_fixed above).
// GRID: the sphere-only variants' walk on the grid form of exact re-treeing (DGrid; vk_trace.h grid_step) instead of a tree.  Staged in
// LDS, the table [cells | refs] takes the items' place (lds_items = its size in 32-byte units).  A failed segment requeues its sample for
// the second launch — also from global memory (walking the tree as handed over in place was tried: with a lane or two per wave on that
// tree nearly every step of the wave pays for both walks, the 1 M-sphere scene ran at half the tree forms' rate).
template <uint32_t F, bool LDS_SCENE, int MINW, bool STATS, bool COST = false, bool GRID = false>
__global__ __launch_bounds__((MINW <= 4 ? 1024 : (MINW == 5 ? 640 : (MINW == 6 ? 768 : 1024))), MINW) void render_kernel(KArgs A_byval) {
    // (MINW == 7: the sphere-only LDS variants' dual launch, 1024- and 768-thread workgroups of the same build: vk_api.hip launch_dual)
    (void)A_byval;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    using Mem = typename std::conditional<LDS_SCENE, LdsMem, GlobalMem>::type;
    // diagnostic counters (STATS build only): phase executions and the lanes that had work in them
    unsigned long long st_box_steps = 0, st_box_lanes = 0, st_prim_execs = 0, st_prim_lanes = 0, st_shade_execs = 0, st_shade_lanes = 0,
        st_sched = 0;
    unsigned long long st_t_box = 0, st_t_light = 0, st_t_heavy = 0, st_t_shade = 0, st_heavy_execs = 0, st_t0 = 0, st_t_total = 0,
        st_t_mat = 0, st_t_refill = 0, st_t_install = 0, st_t1 = 0, st_t_turb = 0, st_t_cold = 0;
    if (STATS) st_t_total = clock64();

    if constexpr ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) {      // the fallback launch of exact re-treeing: nothing to do, nearly always
        KArgsC P = kargs_fresh();
        if (KARG(P, list_mode) == 2u && KARG(P, redo_plan)[2] == 0u) return;
    }
    // ---- LDS layout: [items][spheres][boxes][per wave: cold lane state | tile sums | wave state]
    uint32_t lds_items = 0;
    float *cold;
    unsigned long long *tile_sum;   // the wave's current tile: 64 pixels x 3 fixed-point sums
    uint32_t *wstate;
    uint32_t wave_block;            // offset of this wave's LDS block in the dynamic LDS, in floats
    {
        KArgsC P = kargs_fresh();
        lds_items = LDS_SCENE ? KARG(P, lds_items) : 0u;
        uint32_t lds_spheres = LDS_SCENE ? KARG(P, lds_spheres) : 0u;
        uint32_t lds_boxes = LDS_SCENE ? KARG(P, lds_boxes) : 0u;
        wave_block = 4u * (2u * lds_items + lds_spheres + 2u * lds_boxes) + wave * wave_block_floats<F>();     // in floats from smem
        cold = reinterpret_cast<float *>(smem) + wave_block;
        tile_sum = reinterpret_cast<unsigned long long *>(cold + 64 * ncold<F>());
        wstate = reinterpret_cast<uint32_t *>(cold + 64 * ncold<F>() + 64 * 3 * 2);
        if (lane == 0) {      // for called code: the address of the kernel-argument segment
            uint64_t a = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
            wstate[WS_KARGS] = (uint32_t)a; wstate[WS_KARGS + 1] = (uint32_t)(a >> 32);
        }
        if (LDS_SCENE) {
            if constexpr (GRID) {
                const uint4 *gt = reinterpret_cast<const uint4 *>(KARG(P, S.grid_cells));      // [cells | refs], padded to 32 bytes
                for (uint32_t k = threadIdx.x; k < 2u * lds_items; k += blockDim.x) smem[k] = gt[k];
            } else {
            const uint4 *gi = reinterpret_cast<const uint4 *>(KARG(P, S.items));
            for (uint32_t k = threadIdx.x; k < 2u * lds_items; k += blockDim.x) {
                uint4 h = gi[k];
                if ((k & 1u) && (h.z >> 28) == 0u) h.z <<= LdsMem::ISHIFT;      // an inner item's skip link, in cursor units
                smem[(k >> 1) + ((k & 1u) ? lds_items : 0u)] = h;
            }
            }
            const uint4 *gs = reinterpret_cast<const uint4 *>(KARG(P, S.spheres));
            for (uint32_t k = threadIdx.x; k < lds_spheres; k += blockDim.x) smem[2u * lds_items + k] = gs[k];
            const uint4 *gb = reinterpret_cast<const uint4 *>(KARG(P, S.boxes));
            for (uint32_t k = threadIdx.x; k < 2u * lds_boxes; k += blockDim.x) smem[2u * lds_items + lds_spheres + k] = gb[k];
            __syncthreads();
        }
    }
#ifdef VK_WAVE_TIMES          // (diagnostic builds only, tools/experiments/build_exp.sh -DVK_WAVE_TIMES: the stores cost the production kernels 1 %)
    { KArgsC P = kargs_fresh(); unsigned long long *wt = KARG(P, wave_times);
      if (wt && lane == 0) wt[3u * ((blockIdx.x + (blockDim.x == 1024u ? 0u : gridDim.x)) * 16u + wave)] = wall_clock64(); }
#endif
    // the wave has no unit yet: the first SHADE + REFILL phase pulls one
    tile_sum[lane * 3 + 0] = 0ull; tile_sum[lane * 3 + 1] = 0ull; tile_sum[lane * 3 + 2] = 0ull;
    if (lane == 0) { wstate[WS_TXY] = 0xFFFFFFFFu; wstate[WS_NEXT] = 0u; wstate[WS_TOTAL] = 0u; }

    Lane L;
    __builtin_memset(&L, 0, sizeof(L));     // (the intrinsic: HIP's device memset() is a loop, which keeps a Lane this large in scratch)
    uint32_t cost_t0 = 0;      // probe (COST) build only: when this lane's current sample started
    (void)cost_t0;
    bool need = true;          // lane has no path and wants a sample (false once the launch's units are all handed out)
    bool active = false;       // lane holds a live path
    // Wave-level phase scheduler.  Every lane is in one of four states; each round the
    // wave runs the code of the most populated state with the lanes in it (64-bit ballots
    // + s_bcnt1), so the long box loop, the primitive tests and the (expensive, rare)
    // shading / ray-generation code each execute with as many lanes as possible instead
    // of all being paid for on every iteration:
    //   BOX    pend == 0 and items (or an instance to leave) remain  -> box_step
    //   PRIM   pend != 0                                             -> prim_step
    //   SHADE  live path whose segment is fully traversed            -> shade
    //   NEED   no path; samples remain                               -> start_sample
    // SHADE and NEED run as one phase: a path that ends hands its lane straight to the
    // next sample (ballot + prefix popcount = active-ray compaction).
    // (per-XCD work queues — contiguous image bands per XCD, stealing when empty — were tried for L2 locality on
    // C5: no gain there, -1.7 % on C2, and the two extra live scalars doubled the everything-variant's spills)
    uint32_t shade_defer, prim_weight;
    { KArgsC U = kargs_fresh(); shade_defer = KARG(U, shade_defer); prim_weight = KARG(U, prim_weight); }
    // lanes holding a path / wanting a sample, as wave masks: both only change in the SHADE + REFILL phase
    unsigned long long m_act = 0ull, m_need = ~0ull;
    for (;;) {
        // the lane masks of the four states from compares, combined and counted with scalar instructions (see the BOX loop)
        // primitives come in two weights (sphere/rect ~50 instructions; Boxy, list, medium, instance
        // entry several times that): scheduled separately so cheap tests never pay for heavy ones
        const bool HAS_HEAVY = (F & (VKF_LIST | VKF_MEDIUM | VKF_INSTANCE | VKF_BOX)) != 0;
        const unsigned long long m_pend0 = __builtin_amdgcn_uicmp(L.pend, 0u, 33 /* ne */) & m_act;
        unsigned long long m_trav = __builtin_amdgcn_uicmp(L.i, L.end, 36 /* ult */);
        if (F & VKF_INSTANCE) m_trav |= __builtin_amdgcn_sicmp(L.cur_inst, 0, 39 /* sge */);
        if (GRID) m_trav |= __builtin_amdgcn_uicmp(L.cell, GRID_LAST, 36 /* ult */);
        const unsigned long long m_heavy = HAS_HEAVY ? (heavy_mask<F>(L.pend) & m_pend0) : 0ull;
        const unsigned long long m_light = m_pend0 & ~m_heavy;
        const unsigned long long m_shade = m_act & ~m_pend0 & ~m_trav;
        const uint32_t n_box = (uint32_t)__builtin_popcountll(m_act & ~m_pend0 & m_trav);
        const uint32_t n_heavy = (uint32_t)__builtin_popcountll(m_heavy), n_light = (uint32_t)__builtin_popcountll(m_light);
        const uint32_t n_prim = n_heavy > n_light ? n_heavy : n_light;
        const uint32_t n_sn = (uint32_t)__builtin_popcountll(m_shade | m_need);
        if ((n_box | n_prim | n_sn) == 0) break;
        if (STATS) st_sched++;
        if (n_box >= n_prim * prim_weight && n_box * shade_defer >= n_sn) {
            // ---- BOX: UNROLL steps under a shrinking EXEC mask per exit test, while box lanes are the plurality
            KArgsC P = kargs_fresh();
            DScene S = KARG(P, S);
            Mem M = make_mem<F, LDS_SCENE>(S, lds_items);
            if (STATS) st_t0 = clock64();
            const uint32_t live = n_box + n_heavy + n_light + n_sn;   // lanes only change state here, none appear or vanish
            // steps between two exit tests (compile time: a run-time trip count costs 4-13 %).  With shading deferred the optimum is 3
            // for scenes traversed from LDS (C2: 2 -> -4 %, 4 -> -0.5 %; C4 the same), 2 for sphere-only scenes traversed from global
            // memory (C5 on the tree handed over: 3 / 4 / 5 / 7 -> 706 / 724 / 722 / 703 Msamples/s; on the shorter walks of the rebuilt
            // tree: VK_GLOBAL_SPHERE_UNROLL below) and 5 for the everything-variants (C3: 4 / 5 / 6 / 8 ->
            // 617 / 627 / 622 / 616): the longer a step waits for its item, the less an exit test per step group is worth
            constexpr bool SPHERES = (F & ~(uint32_t)VKF_INTEG_PDF) == 0u;
#ifndef VK_CORNELL_UNROLL
#define VK_CORNELL_UNROLL 3
#endif
#ifndef VK_GLOBAL_SPHERE_UNROLL
// (on the rebuilt trees of exact re-treeing, 1 M spheres, 1 / 2 / 3 / 4 steps per exit test: 1 046 / 1 080 / 1 066 / 1 038 Msamples/s in the
// empirical unit form, round 3; in the near form, round 5, whose walks alternate between the rebuilt and the handed-over tree:
// 2 / 3 / 4 -> 1 263 / 1 276 / 1 254)
#define VK_GLOBAL_SPHERE_UNROLL 3
#endif
            constexpr int UNROLL = ((F & VKF_ALL_SCENE) == VKF_ALL_SCENE)
                ? BOX_UNROLL + 1 : (SPHERES ? (LDS_SCENE ? BOX_UNROLL - 1 : VK_GLOBAL_SPHERE_UNROLL) : VK_CORNELL_UNROLL);
            // The lane masks of the states come straight out of compares (uicmp = v_cmp into an SGPR pair) and are combined and
            // counted with scalar instructions; a ballot of a compound lane boolean goes through a VGPR (v_cndmask 0/1 + v_cmp_ne)
            // for every term.  The lanes that step are the box lanes of the last exit test: their mask is at hand in SGPRs and
            // the inverse ballot — the lane predicate of a mask — is free.
            unsigned long long m_pend, m_lt, m_inst = 0ull;
            auto masks = [&]() {
                m_pend = __builtin_amdgcn_uicmp(L.pend, 0u, 33 /* ne */);
                if constexpr (GRID) m_lt = __builtin_amdgcn_uicmp(L.i, L.end, 36 /* ult */) | __builtin_amdgcn_uicmp(L.cell, GRID_LAST, 36 /* ult */);
                else m_lt = __builtin_amdgcn_uicmp(L.i, range_end<F, Mem>(L, S), 36 /* ult */);
                if (F & VKF_INSTANCE) m_inst = __builtin_amdgcn_sicmp(L.cur_inst, 0, 39 /* sge */);
            };
            masks();
            for (;;) {
                if (F & VKF_INSTANCE) {     // end of an instance's item range: back to the parent space (rare)
                    const unsigned long long m_leave = m_act & ~m_pend & ~m_lt & m_inst;
                    if (m_leave != 0ull) {
                        if (__builtin_amdgcn_inverse_ballot_w64(m_leave)) { cold_load_world_ray<F>(cold, lane, L);
                            leave_instance<F, Mem>(L, S); }
                        masks();
                    }
                }
                bool go = __builtin_amdgcn_inverse_ballot_w64(m_act & ~m_pend & m_lt);
                if (STATS) {        // diagnostic build: same steps one at a time, counting the lanes in each
                    for (int u = 0; u < UNROLL; u++) {
                        st_box_steps += 1; st_box_lanes += lanes_with(go);
                        box_steps<F, Mem, 1>(L, S, M, go);
                        go = active && L.pend == 0u && L.i < range_end<F, Mem>(L, S);
                    }
                } else if constexpr (GRID) {
                    // one grid step per exit test: the next two references of the lane's cell, or the next cell
                    if (go) (void)grid_step(L, S, M);
                } else {
                    box_steps<F, Mem, UNROLL>(L, S, M, go);
                }
                // exit test on wave-uniform counts
                masks();
                const unsigned long long m_prim = m_pend & m_act, m_box = (m_lt | m_inst) & ~m_pend & m_act;
                const uint32_t nb = (uint32_t)__builtin_popcountll(m_box), np = (uint32_t)__builtin_popcountll(m_prim);
                const uint32_t ns = live - nb - np;
                // sphere-only diagnostic: lanes per exit test
                if (STATS && !HAS_HEAVY) { st_heavy_execs += live; st_t_light += np; st_t_heavy += ns; st_prim_execs += 1; }
                // keep stepping while nb != 0, nb >= np * prim_weight and nb * shade_defer >= ns: as sign tests of differences (the
                // counts are < 2^7), which is a third of the scalar instructions of three compares or-ed together
                const int keep1 = (int)nb - (int)(np * prim_weight > 1u ? np * prim_weight : 1u), keep2 = (int)(nb * shade_defer) - (int)ns;
                if ((keep1 | keep2) < 0) {   // another state now has more lanes parked than are stepping
                    // when that state is a LIGHT primitive test (Sphere / MovingSphere / Rect: never draws, never changes the
                    // space), run it right here and keep stepping: saves the scheduler round trip that otherwise follows every
                    // ~10 box steps
                    const unsigned long long m_light = HAS_HEAVY ? (m_prim & ~heavy_mask<F>(L.pend)) : m_prim;
                    const uint32_t nl = (uint32_t)__builtin_popcountll(m_light);
                    // nl != 0, 2 nl >= np, nl * shade_defer >= ns
                    if ((((int)nl - 1) | ((int)(2u * nl) - (int)np) | ((int)(nl * shade_defer) - (int)ns)) >= 0) {
                        if (__builtin_amdgcn_inverse_ballot_w64(m_light)) prim_step<F, Mem>(L, S, M);
                        masks();
                        continue;
                    }
                    break;
                }
            }
            if (STATS) st_t_box += clock64() - st_t0;
        } else if (n_prim * shade_defer >= n_sn) {
            // ---- PRIM: intersect / enter the pending object
            KArgsC P = kargs_fresh();
            DScene S = KARG(P, S);
            Mem M = make_mem<F, LDS_SCENE>(S, lds_items);
            if (STATS) { st_prim_execs++; st_prim_lanes += n_prim; st_t0 = clock64(); if (n_heavy > n_light) st_heavy_execs++; }
            if (__builtin_amdgcn_inverse_ballot_w64(n_heavy > n_light ? m_heavy : m_light)) {
                if (F & VKF_MEDIUM) {    // ConstantMedium::hit draws inside traversal (hittable.rs:473)
                    L.rng.key = (uint64_t)__float_as_uint(cold[CF_KEY * 64 + lane]) |
                                ((uint64_t)__float_as_uint(cold[(CF_KEY + 1) * 64 + lane]) << 32);
                    L.rng.ctr = __float_as_uint(cold[CF_CTR * 64 + lane]);
                }
                prim_step<F, Mem>(L, S, M);
                if (F & VKF_MEDIUM) cold[CF_CTR * 64 + lane] = __uint_as_float(L.rng.ctr);
            }
            if (STATS) { if (n_heavy > n_light) st_t_heavy += clock64() - st_t0; else st_t_light += clock64() - st_t0; }
        } else {
            // ---- SHADE + REFILL
            if (STATS) { st_shade_execs++; st_shade_lanes += n_sn; st_t0 = clock64(); }
            // out of line for the everything-variants (see shade_refill_call); one begin_segment for both kinds of new ray
            // ... and for an 8-waves-per-SIMD build of the sphere-only variants (64 VGPRs hold the traversal loops but not shading), which
            // global-memory scenes ran until exact re-treeing halved their walks: now seven waves with the phase inline (vk_api.hip
            // launch_variant), and no instance of the kernel has MINW == 8
            constexpr bool SPLIT = ((F & VKF_ALL_SCENE) == VKF_ALL_SCENE || MINW == 8) && !STATS;
            const bool is_shade = __builtin_amdgcn_inverse_ballot_w64(m_shade);
            bool touched = false, fresh = false;
            bool early = false;       // exact re-treeing: this segment's winner may depend on the visiting order
            if constexpr ((F & ~(uint32_t)VKF_INTEG_PDF) == 0u) {
                KArgsC P = kargs_fresh();
                DScene S = KARG(P, S);
                if (S.t_pad > 0.0f) {      // (wave-uniform)
                    Mem M = make_mem<F, LDS_SCENE>(S, lds_items);
                    bool on_ref = false;   // the lane has just walked the tree as handed over: its answer stands
                    if constexpr (!LDS_SCENE) {
                        // (bit 31 of the depth word: walked again after an early winner; depth 1 under DScene::primary_ref: a primary ray
                        // that begin_segment started on the tree as handed over)
                        const uint32_t dw = __float_as_uint(cold[CF_DEPTH * 64 + lane]);
                        on_ref = (dw >> 31) != 0u || (S.primary_ref != 0u && S.walk_start != 0u && dw == 1u);
                    }
                    if (is_shade && !on_ref) early = segment_unsafe<F, Mem>(L, S, M);
                }
            }
            if constexpr (SPLIT) {
                ShadeIo io;
                io.flags = (is_shade ? 1u : 0u) | (active ? 2u : 0u) | (need ? 4u : 0u) | (early ? 64u : 0u);
                io.T = L.T; io.best_prim = L.best_prim; io.best_inst = L.best_inst; io.best_aux = L.best_aux;
                io.o = L.o; io.d = L.d; io.time = L.time; io.cost_t0 = cost_t0;
                io = shade_refill_call<F, LDS_SCENE, COST>(io, lds_items, wave_block);
                active = (io.flags & 2u) != 0u; need = (io.flags & 4u) != 0u; fresh = (io.flags & 8u) != 0u;
                const bool rearm = (io.flags & 32u) != 0u;      // exact re-treeing: the same ray again, on the tree as handed over
                cost_t0 = io.cost_t0;
                if (fresh | rearm) {
                    KArgsC P = kargs_fresh();
                    DScene S = KARG(P, S);
                    // (the callee stored the path state, new world ray included)
                    begin_segment<Mem::ISHIFT, fused_box<F, Mem>(), spheres_only<F>()>(L, S, io.o, io.d, io.time, rearm);
                }
            } else {
                PhaseClocks clk;
                bool rearm = false;
                shade_refill_body<F, LDS_SCENE, STATS, COST>(L, is_shade, early, active, need, fresh, touched, rearm, cost_t0,
                    kargs_fresh(), cold,
                    tile_sum, wstate, lane, lds_items, clk);
                if (STATS) { st_t_mat += clk.mat; st_t_refill += clk.refill; st_t_turb += clk.turb; st_t_cold += clk.cold; st_t1 = clock64(); }
                if (fresh | rearm) {
                    KArgsC P = kargs_fresh();
                    DScene S = KARG(P, S);
                    // one copy of the exact reciprocals for both kinds of new ray
                    begin_segment<Mem::ISHIFT, fused_box<F, Mem>(), spheres_only<F>()>(L, S, L.wo, L.wd, L.time, rearm);
                }
                if (active && touched) cold_store_path<F>(cold, lane, L);
                if (STATS) st_t_install += clock64() - st_t1;
            }
            m_act = __builtin_amdgcn_ballot_w64(active); m_need = __builtin_amdgcn_ballot_w64(need);
            if (STATS) st_t_shade += clock64() - st_t0;
        }
    }
    {   // the last unit's sums
        KArgsC P = kargs_fresh();
#ifdef VK_WAVE_TIMES
        unsigned long long *wt = KARG(P, wave_times);
        if (wt && lane == 0) wt[3u * ((blockIdx.x + (blockDim.x == 1024u ? 0u : gridDim.x)) * 16u + wave) + 2u] = wall_clock64();
#endif
        flush_tile_sums(tile_sum, KARG(P, accum), __builtin_amdgcn_readfirstlane(wstate[WS_TXY]), lane, KARG(P, C.width),
            KARG(P, C.height));
    }
    if (STATS) {
        KArgsC P = kargs_fresh();
        unsigned long long *ps = KARG(P, phase_stats);
        if (ps && lane == 0) {
            atomicAdd(&ps[0], st_box_steps); atomicAdd(&ps[1], st_box_lanes); atomicAdd(&ps[2], st_prim_execs);
            atomicAdd(&ps[3], st_prim_lanes);
            atomicAdd(&ps[4], st_shade_execs); atomicAdd(&ps[5], st_shade_lanes); atomicAdd(&ps[6], st_sched);
            atomicAdd(&ps[7], st_heavy_execs);
            atomicAdd(&ps[8], st_t_box); atomicAdd(&ps[9], st_t_light); atomicAdd(&ps[10], st_t_heavy); atomicAdd(&ps[11], st_t_shade);
            atomicAdd(&ps[12], (unsigned long long)(clock64() - st_t_total));
            atomicAdd(&ps[13], st_t_mat); atomicAdd(&ps[14], st_t_refill); atomicAdd(&ps[15], st_t_install);
            atomicAdd(&ps[16], st_t_turb); atomicAdd(&ps[17], st_t_cold);
        }
    }
}

// Between the two launches of exact re-treeing (ONE block of REDO_REGIONS threads): plan[1] = samples queued (vk_stats), plan[2] = entries
// that did not fit their queue (must be 0), plan[3] = entries per work unit of the second launch — 64 (one sample per lane: a short list
// then reaches every wave and the launch lasts about as long as its longest path) up to REDO_UNIT for long lists — and plan[0] = units of
// that size in the fullest queue (the second launch's units are REDO_REGIONS x that).
__global__ void redo_plan_kernel(const uint32_t *count, uint32_t cap, uint32_t *plan, uint32_t n_waves) {
    __shared__ uint32_t s_total, s_max, s_lost;
    const uint32_t r = threadIdx.x;
    if (r == 0) { s_total = 0; s_max = 0; s_lost = 0; }
    __syncthreads();
    const uint32_t c = r < REDO_REGIONS ? count[r * REDO_COUNT_STRIDE] : 0u;
    const uint32_t kept = c < cap ? c : cap;
    atomicAdd(&s_total, kept); atomicMax(&s_max, kept);
    if (c > cap) atomicAdd(&s_lost, c - cap);
    __syncthreads();
    if (r == 0) {
        uint32_t unit = 64u;
        while (unit < REDO_UNIT && (uint64_t)s_total > (uint64_t)unit * n_waves * 2u) unit *= 2u;
        plan[0] = (s_max + unit - 1u) / unit; plan[1] = s_total; plan[2] = s_lost; plan[3] = unit;
    }
}

// Behind the second launch: if a queue overflowed (plan[2] != 0) the frame is incomplete — the sums and the unit counter are cleared and the
// fallback launch (list_mode = 2) renders the partition again on the tree as handed over.  Nearly always: nothing.
__global__ void redo_reset_kernel(const uint32_t *plan, unsigned long long *accum, size_t n_words, uint32_t *counter) {
    if (plan[2] == 0u) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { counter[0] = 0u; counter[2] = 0u; counter[3] = 0u; }      // the unit counter and the clamped-sample count
    for (size_t k = i; k < n_words; k += (size_t)gridDim.x * blockDim.x) accum[k] = 0ull;
}

// ---- heavy-first tile order (bucket sort of the probe's per-tile times, dearest first).
// 8 buckets per octave of cost; the order inside a bucket is arbitrary, which is fine: any order renders the same image.
constexpr uint32_t ORDER_BUCKETS = 256;
__device__ __forceinline__ uint32_t cost_bucket(uint32_t c) {
    if (c < 8u) return c;
    uint32_t msb = 31u - (uint32_t)__builtin_clz(c);
    uint32_t b = (msb - 2u) * 8u + ((c >> (msb - 3u)) & 7u);
    return b < ORDER_BUCKETS ? b : ORDER_BUCKETS - 1u;
}
__global__ void order_hist_kernel(const uint32_t *cost, uint32_t n_local, uint32_t tile_rank, uint32_t tile_world, uint32_t *hist) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_local) atomicAdd(&hist[cost_bucket(cost[tile_rank + i * tile_world])], 1u);
}
__global__ void order_scan_kernel(uint32_t *hist) {      // one thread: start offset of every bucket, dearest bucket first
    uint32_t run = 0;
    for (int b = (int)ORDER_BUCKETS - 1; b >= 0; b--) { uint32_t c = hist[b]; hist[b] = run; run += c; }
}
__global__ void order_scatter_kernel(uint32_t *cost, uint32_t n_local, uint32_t tile_rank, uint32_t tile_world, uint32_t *hist,
    uint32_t *order) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_local) return;
    uint32_t t = tile_rank + i * tile_world;
    order[atomicAdd(&hist[cost_bucket(cost[t])], 1u)] = i;
}

// pixel mean = fixed-point sum / spp (main.rs:196), for the pixels of this call's tile partition
__global__ void resolve_kernel(const long long *accum, float *out, uint32_t width, uint32_t height, uint32_t spp,
                               uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world) {
    uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n_pixels = width * height;
    if (pix >= n_pixels) return;
    uint32_t x = pix % width, y = pix / width;
    uint32_t tile = (y / TILE) * tiles_x + (x / TILE);
    if (tile % tile_world != tile_rank) return;
    float n = (float)spp;
    const long long *a = accum + (size_t)pix * 3;
    const float inv_scale = 1.0f / ACCUM_SCALE;
    out[(size_t)pix * 3 + 0] = ((float)a[0] * inv_scale) / n;
    out[(size_t)pix * 3 + 1] = ((float)a[1] * inv_scale) / n;
    out[(size_t)pix * 3 + 2] = ((float)a[2] * inv_scale) / n;
}

// Progressive rendering (vk_progress_step): behind a window's launches, for the pixels of this call's tile partition, ONE pass that
//   * adds the window's fixed-point sums (accum, zeroed per window) into the handle's running sums — integer adds, exact: after any
//     sequence of windows the running sums are the one-shot frame's sums of the same samples, bit for bit;
//   * writes the running mean with resolve_kernel's arithmetic, so that the image is the one vk_render gives at spp = samples done;
//   * with error moments on (m2 != null), adds n_j m_j^2 per component: m_j = the window's own mean, from its exact sum (batch means,
//     vk_progress_stderr).
// Thread 0 also adds the window's clamped-sample count (counter block bytes 8..15) to the handle's.
__global__ void accumulate_resolve_kernel(const long long *accum, long long *run, double *m2, float *out, uint32_t width, uint32_t height,
                                          uint32_t window, uint32_t done, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                          const unsigned long long *win_clamped, unsigned long long *run_clamped) {
    uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix == 0) *run_clamped += *win_clamped;
    uint32_t n_pixels = width * height;
    if (pix >= n_pixels) return;
    uint32_t x = pix % width, y = pix / width;
    uint32_t tile = (y / TILE) * tiles_x + (x / TILE);
    if (tile % tile_world != tile_rank) return;
    float n = (float)done;
    const float inv_scale = 1.0f / ACCUM_SCALE;
    for (int c = 0; c < 3; c++) {
        const size_t i = (size_t)pix * 3 + c;
        const long long w = accum[i], r = run[i] + w;
        run[i] = r;
        out[i] = ((float)r * inv_scale) / n;
        if (m2) { const double s = (double)w * (1.0 / (double)ACCUM_SCALE); m2[i] += s * s / (double)window; }
    }
}

// ---- adaptive progressive rendering (vk_progress_set_adaptive) ---------------------------------------------------------------------
// Per local tile slot i of a part (tile = tile_rank + i * tile_world): tile_n[i] = the samples a CONVERGED tile froze with (0 = still
// active, its count is the handle's samples done), tile_k[i] = its windows.  A window renders the active tiles only (KArgs::tile_order
// = the active list, KArgs::active_count = its length), so a frozen tile's running sums stop at tile_n[i] samples.

// Compaction, 1: active slots per 1024-slot block of the tile order (ord = the probe's dearest-first order, or null = raster order).
__global__ void __launch_bounds__(1024) adaptive_count_kernel(const uint32_t *ord, const uint32_t *tile_n, uint32_t n_local,
                                                              uint32_t *block_count) {
    __shared__ uint32_t wc[16];
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool act = i < n_local && tile_n[ord ? ord[i] : i] == 0u;
    const unsigned long long m = __ballot(act);
    if (lane == 0) wc[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < 16; k++) s += wc[k];
        block_count[blockIdx.x] = s;
    }
}

// Compaction, 2: every block adds up the counts of the blocks before it and writes its active slots in order behind them (stable:
// the list is the order filtered, the same on every run); the last block writes the list's length.
__global__ void __launch_bounds__(1024) adaptive_scatter_kernel(const uint32_t *ord, const uint32_t *tile_n, uint32_t n_local,
                                                                const uint32_t *block_count, uint32_t *list, uint32_t *count) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t wc[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t s = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 1024u) s += block_count[b];
    part[threadIdx.x] = s;
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    const uint32_t slot = i < n_local ? (ord ? ord[i] : i) : 0u;
    const bool act = i < n_local && tile_n[slot] == 0u;
    const unsigned long long m = __ballot(act);
    if (lane == 0) wc[w] = (uint32_t)__popcll(m);
    __syncthreads();
    for (uint32_t h = 512u; h > 0u; h >>= 1) {          // the blocks before this one: a tree sum (integers: exact in any order)
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    uint32_t base = part[0];
    for (uint32_t k = 0; k < w; k++) base += wc[k];
    if (act) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = slot;
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) {
        uint32_t t = part[0];
        for (int k = 0; k < 16; k++) t += wc[k];
        *count = t;
    }
}

// The resolve of an adaptive window: accumulate_resolve_kernel for the active tiles (mean over `done` samples), and for the frozen ones
// their running sums over tile_n samples — which the window did not touch (it rendered no unit of theirs: accum is 0 there).  Every
// pixel of the partition is written, so that every preview is complete.
__global__ void adaptive_resolve_kernel(const long long *accum, long long *run, double *m2, float *out, uint32_t width, uint32_t height,
                                        uint32_t window, uint32_t done, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                        const uint32_t *tile_n, const unsigned long long *win_clamped, unsigned long long *run_clamped) {
    uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix == 0) *run_clamped += *win_clamped;
    uint32_t n_pixels = width * height;
    if (pix >= n_pixels) return;
    uint32_t x = pix % width, y = pix / width;
    uint32_t tile = (y / TILE) * tiles_x + (x / TILE);
    if (tile % tile_world != tile_rank) return;
    const uint32_t frozen = tile_n[tile / tile_world];
    const float inv_scale = 1.0f / ACCUM_SCALE;
    if (frozen != 0u) {
        const float n = (float)frozen;
        for (int c = 0; c < 3; c++) out[(size_t)pix * 3 + c] = ((float)run[(size_t)pix * 3 + c] * inv_scale) / n;
        return;
    }
    float n = (float)done;
    for (int c = 0; c < 3; c++) {
        const size_t i = (size_t)pix * 3 + c;
        const long long w = accum[i], r = run[i] + w;
        run[i] = r;
        out[i] = ((float)r * inv_scale) / n;
        if (m2) { const double s = (double)w * (1.0 / (double)ACCUM_SCALE); m2[i] += s * s / (double)window; }
    }
}

// The judge, behind the adaptive resolve: one wave per active tile, one lane per pixel.  A pixel has converged when for every component
//   v <= (abs_tol + rel_tol |mean|)^2,   mean = run / 2^26 / N,   v = (m2 - N mean^2) / ((k - 1) N)
// in double, with vk_progress_stderr's operation order (built without contraction: a numpy restatement reproduces every decision).  A
// tile converges when all its in-image pixels have (lanes outside the image do not vote) and the gates (min_samples, min_steps: `gate`)
// are met; it is then frozen at (done, steps).  The tiles left active, and their in-image pixels, are counted into left[0] and
// left_px (zeroed before): the host sizes the next window from them.
__global__ void adaptive_judge_kernel(const long long *run, const double *m2, uint32_t width, uint32_t height, uint32_t tiles_x,
                                      uint32_t tile_rank, uint32_t tile_world, uint32_t n_local, uint32_t done, uint32_t steps, uint32_t gate,
                                      float abs_tol, float rel_tol, uint32_t *tile_n, uint32_t *tile_k, uint32_t *left,
                                      unsigned long long *left_px) {
    const uint32_t slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (slot >= n_local || tile_n[slot] != 0u) return;         // (uniform per wave)
    const uint32_t tile = tile_rank + slot * tile_world;
    const uint32_t px = (tile % tiles_x) * TILE + (lane & 7u), py = (tile / tiles_x) * TILE + (lane >> 3);
    const bool inside = px < width && py < height;
    bool conv = true;
    if (inside && gate) {
        const double N = (double)done, k = (double)steps, at = (double)abs_tol, rt = (double)rel_tol;
        for (int c = 0; c < 3; c++) {
            const size_t i = ((size_t)py * width + px) * 3 + c;
            const double mean = (double)run[i] / (double)ACCUM_SCALE / N;
            const double v = (m2[i] - N * mean * mean) / ((k - 1.0) * N);
            const double tol = at + rt * fabs(mean);
            conv = conv && v <= tol * tol;
        }
    }
    const unsigned long long in_mask = __ballot(inside), conv_mask = __ballot(conv);
    if (lane != 0) return;
    if (gate && conv_mask == ~0ull) {
        tile_n[slot] = done; tile_k[slot] = steps;
    } else {
        atomicAdd(left, 1u);
        atomicAdd(left_px, (unsigned long long)__popcll(in_mask));
    }
}

// Vec3::to_color (vec3.rs:44-61): sqrt gamma, hand-written clamp (NaN falls through it), *256, `as u32`
// (saturating; NaN -> 0), for one component
__device__ __forceinline__ uint8_t to_color_u8(float x) {
    float v = sqrtf(x);
    float cl = v < 0.0f ? 0.0f : (v > 0.999f ? 0.999f : v);
    return (uint8_t)vk::sat_u32(256.0f * cl);
}
// whole image: Vec3::to_color + top-down rows (main.rs:209)
__global__ void to_color_kernel(const float *rgb, uint32_t width, uint32_t height, uint8_t *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)width * height * 3;
    if (i >= n) return;
    uint32_t c = (uint32_t)(i % 3);
    size_t pix = i / 3;
    uint32_t x = (uint32_t)(pix % width), row = (uint32_t)(pix / width);
    uint32_t y = height - 1 - row;
    out[i] = to_color_u8(rgb[((size_t)y * width + x) * 3 + c]);
}

// ---- first-hit buffers (vk_render_aov): albedo, normal, depth and coverage of the primary rays of samples
// [first_sample, first_sample + C.spp) of every pixel of this call's tile partition.  One 8x8 tile per wave (coherent primary rays,
// each tile row's eight lanes store 96 contiguous bytes), the samples in increasing order inside the lane, f32 sums: the result does not
// depend on the launch shape.  The walk is vk_trace.h's per-lane one (begin_segment / traverse_step / build_record) on GlobalMem.
struct AovArgs {
    DScene S;                // a tree view (vk_api.hip aov_view): grid.nu == 0, no rebuilt-form gates
    RenderConsts C;          // C.spp = the window's length
    float *albedo, *normal, *depth, *coverage;   // f32, y up, each may be null
    uint32_t first_sample, tiles_x, tile_rank, tile_world, n_local;
};
constexpr int AOV_BLOCK = 256;       // 4 waves = 4 tiles per workgroup
template <uint32_t F>
__global__ __launch_bounds__(AOV_BLOCK) void aov_kernel(AovArgs A) {
    const uint32_t lane = threadIdx.x & 63u, local = blockIdx.x * (AOV_BLOCK / 64) + (threadIdx.x >> 6);
    if (local >= A.n_local) return;
    const uint32_t tile = A.tile_rank + local * A.tile_world;
    const uint32_t x = (tile % A.tiles_x) * TILE + (lane & 7u), y = (tile / A.tiles_x) * TILE + (lane >> 3);
    if (x >= A.C.width || y >= A.C.height) return;
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    V3 sa = v3s(0.0f), sn = v3s(0.0f);
    float sd = 0.0f;
    uint32_t hits = 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < A.C.spp; k++) {
        Lane L;
        V3 a, n; float dp; bool h;
        if (!aov_sample<F, GlobalMem>(L, A.S, M, A.C, x, y, A.first_sample + k, a, n, dp, h)) continue;    // dropped: counts in n only
        sa = sa + a; sn = sn + n;
        if (h) { sd += dp; hits++; }
    }
    const float fn = (float)A.C.spp;
    const size_t pix = (size_t)y * A.C.width + x;
    if (A.albedo) { A.albedo[pix * 3 + 0] = sa.x / fn; A.albedo[pix * 3 + 1] = sa.y / fn; A.albedo[pix * 3 + 2] = sa.z / fn; }
    if (A.normal) { A.normal[pix * 3 + 0] = sn.x / fn; A.normal[pix * 3 + 1] = sn.y / fn; A.normal[pix * 3 + 2] = sn.z / fn; }
    if (A.depth) A.depth[pix] = hits ? sd / (float)hits : INFINITY;
    if (A.coverage) A.coverage[pix] = (float)hits / fn;
}

// ---- specular guides (vk_render_guides): the first-hit kernel's launch shape, tile walk and aggregation around vk_trace.h guide_sample,
// whose bounce loop runs inside the lane (a tile's lanes stay together through a large mirror or glass sphere).  bounces: the
// continuations of the kept samples, summed as integers (at most 8 * 2^26), over (float)n.
struct GuideArgs {
    AovArgs A;
    float *bounces;          // f32, y up, may be null
    uint32_t max_bounces; float fuzz_max;
};
template <uint32_t F>
__global__ __launch_bounds__(AOV_BLOCK) void specular_guides_kernel(GuideArgs G) {
    const AovArgs &A = G.A;
    const uint32_t lane = threadIdx.x & 63u, local = blockIdx.x * (AOV_BLOCK / 64) + (threadIdx.x >> 6);
    if (local >= A.n_local) return;
    const uint32_t tile = A.tile_rank + local * A.tile_world;
    const uint32_t x = (tile % A.tiles_x) * TILE + (lane & 7u), y = (tile / A.tiles_x) * TILE + (lane >> 3);
    if (x >= A.C.width || y >= A.C.height) return;
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    // the running sums live in private memory between samples (touched once per sample, outside the walk), not in registers across it
    volatile float sum[7];
    volatile uint32_t cnt[2];
    for (int i = 0; i < 7; i++) sum[i] = 0.0f;
    cnt[0] = 0u; cnt[1] = 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < A.C.spp; k++) {
        Lane L;
        V3 a, n; float dp; bool h; uint32_t b;
        const bool kept = guide_sample<F, GlobalMem>(L, A.S, M, A.C, G.max_bounces, G.fuzz_max, x, y, A.first_sample + k, a, n, dp, h, b);
        if (!kept) continue;                                   // dropped: counts in n only
        sum[0] = sum[0] + a.x; sum[1] = sum[1] + a.y; sum[2] = sum[2] + a.z;
        sum[3] = sum[3] + n.x; sum[4] = sum[4] + n.y; sum[5] = sum[5] + n.z;
        cnt[1] = cnt[1] + b;
        if (h) { sum[6] = sum[6] + dp; cnt[0] = cnt[0] + 1u; }
    }
    const V3 sa = v3(sum[0], sum[1], sum[2]), sn = v3(sum[3], sum[4], sum[5]);
    const float sd = sum[6];
    const uint32_t hits = cnt[0], sb = cnt[1];
    const float fn = (float)A.C.spp;
    const size_t pix = (size_t)y * A.C.width + x;
    if (A.albedo) { A.albedo[pix * 3 + 0] = sa.x / fn; A.albedo[pix * 3 + 1] = sa.y / fn; A.albedo[pix * 3 + 2] = sa.z / fn; }
    if (A.normal) { A.normal[pix * 3 + 0] = sn.x / fn; A.normal[pix * 3 + 1] = sn.y / fn; A.normal[pix * 3 + 2] = sn.z / fn; }
    if (A.depth) A.depth[pix] = hits ? sd / (float)hits : INFINITY;
    if (A.coverage) A.coverage[pix] = (float)hits / fn;
    if (G.bounces) G.bounces[pix] = (float)sb / fn;
}

// ---- ray queries (vk_trace_rays): vk_trace.h trace_ray for rays read from memory, one ray per lane, 64 consecutive rays per wave.  A
// lane reads its vk_ray as two 16-byte loads and writes its vk_hit as four 16-byte stores.  No LDS, no atomics: ray i's result depends
// on (scene, ray i, seed, first_index + i) alone.  The walk is aov_kernel's, on the same tree view.
struct TraceArgs {
    DScene S;                // a tree view (vk_api.hip aov_view)
    DProvenance P;
    const float4 *rays;      // vk_ray[n_rays]
    uint4 *hits;             // vk_hit[n_rays]
    uint64_t seed, first_index, n_rays;
};
template <uint32_t F>
__global__ __launch_bounds__(AOV_BLOCK) void trace_rays_kernel(TraceArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * AOV_BLOCK + threadIdx.x;
    if (i >= A.n_rays) return;
    const float4 r0 = A.rays[i * 2u], r1 = A.rays[i * 2u + 1u];
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    Lane L;
    RayHit H;
    trace_ray<F, GlobalMem>(L, A.S, M, A.P, v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z), r1.w, r0.w, ray_seed(A.seed, A.first_index + i), H);
    uint32_t w[16];
    hit_words(H, w);
    uint4 *out = A.hits + i * 4u;
    out[0] = make_uint4(w[0], w[1], w[2], w[3]);
    out[1] = make_uint4(w[4], w[5], w[6], w[7]);
    out[2] = make_uint4(w[8], w[9], w[10], w[11]);
    out[3] = make_uint4(w[12], w[13], w[14], w[15]);
}

// ---- occlusion queries (vk_trace_occluded): vk_trace.h occluded_ray for rays read from memory, one byte per ray.  Any-hit walks are
// ragged — a ray that starts inside a box it hits ends in a few steps, a miss walks its whole candidate set — and with one ray per lane a
// wave costs its slowest ray.  REFILL: a wave owns rays [wave * 64 * k, (wave + 1) * 64 * k) and hands them to its lanes as they fall
// idle: the idle lanes' ballot, each one's rank in it (mbcnt), a wave-uniform cursor advanced by the popcount — plain C++, the cursor in
// a scalar register because every operand is uniform.  The wave then steps its walking lanes and comes back to the claim once `t` lanes
// are idle and rays remain.  A lane loads its ray as two 16-byte loads and stores its byte at the ray's own index.  No LDS, no atomics:
// ray i's byte depends on (scene, ray i, seed, first_index + i) alone, so which lane walked it when cannot show.  !REFILL: one ray per
// lane, trace_rays_kernel's shape (the A/B partner).  k and t are launch arguments so that tools/occlusion_report.py can sweep them;
// OCC_K and OCC_T are the defaults.
struct OcclusionArgs {
    DScene S;                // a tree view (vk_api.hip aov_view)
    const float4 *rays;      // vk_ray[n_rays]
    uint8_t *occluded;       // [n_rays]
    uint64_t seed, first_index, n_rays;
    uint32_t k, t;           // REFILL only: rays per lane of a wave's block (>= 1), idle lanes that send the wave back to the claim (1..64)
};
constexpr uint32_t OCC_K = 8u, OCC_T = 16u;
// The form vk_trace_occluded launches (the other one: the debug library only).  One ray per lane: on the MI355X the refill form was slower
// on every batch of tools/occlusion_report.py, at every (k, t) swept (Occlusion queries: a wave that owns 64 * k rays leaves
// the machine k times fewer waves to hide the walk's memory latency with, which costs more than the idle lanes it fills).
constexpr bool OCC_PRODUCTION_REFILL = false;
template <uint32_t F, bool REFILL>
__global__ __launch_bounds__(AOV_BLOCK) void occlusion_kernel(OcclusionArgs A) {
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    if constexpr (!REFILL) {
        const uint64_t i = (uint64_t)blockIdx.x * AOV_BLOCK + threadIdx.x;
        if (i >= A.n_rays) return;
        const float4 r0 = A.rays[i * 2u], r1 = A.rays[i * 2u + 1u];
        Lane L;
        A.occluded[i] = occluded_ray<F, GlobalMem>(L, A.S, M, v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z), r1.w, r0.w,
                                                   ray_seed(A.seed, A.first_index + i)) ? 1u : 0u;
    } else {
        // wave-uniform: the block's first ray, its length, how many of its rays have been handed out
        const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (AOV_BLOCK / 64) + (threadIdx.x >> 6));
        const uint64_t per_wave = 64ull * A.k, first = (uint64_t)wave * per_wave;
        if (first >= A.n_rays) return;
        const uint32_t count = (uint32_t)(A.n_rays - first < per_wave ? A.n_rays - first : per_wave);
        uint32_t next = 0u;
        // (the block's own base pointers and seed: ray_seed(seed, first_index + first + m) = ray_seed(wseed, m) in wrapping u64)
        const float4 *wrays = A.rays + first * 2u;
        uint8_t *wout = A.occluded + first;
        const uint64_t wseed = ray_seed(A.seed, A.first_index + first);
        // A lane is idle when its Lane has nothing left to ask (occlusion_walking is false): at the start, after its ray's byte is stored.
        Lane L;
        L.i = 0u; L.end = 0u; L.pend = 0u; L.cur_inst = -1; L.cell = GRID_DONE; L.best_prim = 0u;
        uint32_t mine = 0u;          // the ray this lane walks, counted from `first`
        for (;;) {
            const bool idle_lane = !occlusion_walking(L);
            const unsigned long long idle = __ballot(idle_lane);
            if (next < count && (uint32_t)__popcll(idle) >= A.t) {
                // the claim: the idle lanes take rays first + next, first + next + 1, ... in lane order
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (idle_lane && next + rank < count) {
                    mine = next + rank;
                    const float4 r0 = wrays[mine * 2u], r1 = wrays[mine * 2u + 1u];
                    const bool begun = occlusion_begin<F, GlobalMem>(L, A.S, v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z), r1.w, r0.w,
                                                                     ray_seed(wseed, mine));
                    // decided without a step (the tmax guard left L idle as it was; an empty world, a dead ray): not occluded
                    if (!begun || !occlusion_walking(L)) wout[mine] = 0u;
                }
                const uint32_t taken = (uint32_t)__popcll(idle);
                next = count - next < taken ? count : next + taken;
            } else if (idle == ~0ull) {
                break;               // nothing walks and nothing is left (every wave of a launch is a full one)
            }
            if (occlusion_walking(L)) {
                traverse_step<F, GlobalMem>(L, A.S, M);
                if (!occlusion_walking(L)) wout[mine] = L.best_prim != 0u ? 1u : 0u;
            }
        }
    }
}

// ---- tile slabs: the pixels of one tile partition (tiles t = rank + i*world, i = 0..n_local) packed tile by tile,
// 64 pixel slots per tile, 3 components per slot.  A multi-device scene moves one slab per device to devices[0]
// (the path's only exchange) and de-interleaves it there; RGB8 output packs bytes (to_color fused: 4x less traffic).
enum : int { TM_PACK_F32 = 0, TM_PACK_U8 = 1, TM_UNPACK_F32 = 2, TM_UNPACK_U8 = 3, TM_CONVERT_U8 = 4, TM_ZERO_F32 = 5, TM_ZERO_U8 = 6 };
//   TM_PACK_*     fb (f32, y up) -> slab          TM_UNPACK_F32  slab -> fb (f32, y up)
//   TM_UNPACK_U8  slab (u8) -> rgb8 image, top row first          TM_CONVERT_U8  fb (f32) -> rgb8 image, this partition only
//   TM_ZERO_*     this partition's pixels := 0 (max_depth 0: every sample is (0,0,0), main.rs:126-128)
template <int MODE>
__global__ void tile_move_kernel(const void *src, void *dst, uint32_t width, uint32_t height, uint32_t tiles_x,
                                 uint32_t tile_rank, uint32_t tile_world, uint32_t n_local) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // slab slot: local tile * 64 + pixel slot
    if (idx >= (size_t)n_local * 64u) return;
    uint32_t i = (uint32_t)(idx >> 6), q = (uint32_t)(idx & 63u);
    uint32_t tile = tile_rank + i * tile_world;
    uint32_t px = (tile % tiles_x) * TILE + (q & 7u), py = (tile / tiles_x) * TILE + (q >> 3);
    if (px >= width || py >= height) return;
    size_t up = ((size_t)py * width + px) * 3, down = ((size_t)(height - 1 - py) * width + px) * 3, sl = idx * 3;
    const float *sf = reinterpret_cast<const float *>(src); const uint8_t *sb = reinterpret_cast<const uint8_t *>(src);
    float *df = reinterpret_cast<float *>(dst); uint8_t *db = reinterpret_cast<uint8_t *>(dst);
    for (int c = 0; c < 3; c++) {
        if (MODE == TM_PACK_F32) df[sl + c] = sf[up + c];
        else if (MODE == TM_PACK_U8) db[sl + c] = to_color_u8(sf[up + c]);
        else if (MODE == TM_UNPACK_F32) df[up + c] = sf[sl + c];
        else if (MODE == TM_UNPACK_U8) db[down + c] = sb[sl + c];
        else if (MODE == TM_CONVERT_U8) db[down + c] = to_color_u8(sf[up + c]);
        else if (MODE == TM_ZERO_F32) df[up + c] = 0.0f;
        else db[down + c] = 0;
    }
}

// ---- the denoiser (vk_denoise): an edge-avoiding, variance-guided a-trous wavelet filter over one frame, f32, unfused, in the order the
// header (include/vecchio_amd.h) writes down; tests/denoise_ref.py restates it in numpy and the results agree bit for bit.
//   P[pixel] = (I_r, I_g, I_b, V)   demodulated colour and the variance of its luminance; V = -1 marks an INVALID pixel (V is >= 0 or NaN
//                                   otherwise), which is also what the staged form stores for a slot outside the image
//   G[pixel] = (n_x, n_y, n_z, z)   unit normal, (0,0,0) = no normal (a unit vector is never that); depth, +inf = nothing hit
//   S[pixel] = (g_x, g_y)           the depth slope
// denoise_prepare_kernel packs them, one level kernel per pass reads P (ping) and writes P (pong); the last pass remodulates into `out`.
constexpr uint32_t DN_HAS_STDERR = 1u, DN_HAS_ALBEDO = 2u, DN_HAS_NORMAL = 4u, DN_HAS_DEPTH = 8u, DN_LAST = 16u;
struct DnArgs {
    const float4 *Pin; float4 *Pout; float4 *G; float2 *S;          // (prepare writes Pout, G and S)
    const float *color, *stderr3, *albedo, *normal, *depth;         // prepare: all five; the last level: color and albedo
    float *out;                                                     // the last level
    uint32_t width, height, flags, normal_squarings;
    int s;                                                          // tap spacing of this level
    float sigma_l, sigma_z, albedo_floor;
};
constexpr int DN_BLOCK = 256, DN_SX = 64, DN_R = 4;                 // a workgroup: DN_R rows of DN_SX pixels, one wave per row

__device__ __forceinline__ bool dn_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// E(x) = max(0, 1 - x/8)^8: a compact-support stand-in for exp(-x); fmaxf drops a NaN, so E(NaN) = 0
__device__ __forceinline__ float dn_falloff(float x) {
    float t = fmaxf(0.0f, 1.0f - x * 0.125f);
    t = t * t; t = t * t;
    return t * t;
}

__global__ __launch_bounds__(DN_BLOCK) void denoise_prepare_kernel(DnArgs A) {
    const int x = (int)(blockIdx.x * DN_SX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * DN_R + (threadIdx.x >> 6));
    const int w = (int)A.width, h = (int)A.height;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * A.width + x;
    const float c0 = A.color[p * 3], c1 = A.color[p * 3 + 1], c2 = A.color[p * 3 + 2];
    bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2);
    float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
    if (A.flags & DN_HAS_ALBEDO) {
        a0 = fmaxf(A.albedo[p * 3], A.albedo_floor); a1 = fmaxf(A.albedo[p * 3 + 1], A.albedo_floor);
        a2 = fmaxf(A.albedo[p * 3 + 2], A.albedo_floor);
    }
    float V = 0.0f;
    if (A.flags & DN_HAS_STDERR) {
        const float e0 = A.stderr3[p * 3], e1 = A.stderr3[p * 3 + 1], e2 = A.stderr3[p * 3 + 2];
        valid = valid && dn_finite(e0) && dn_finite(e1) && dn_finite(e2);
        const float sd = dn_lum(e0 / a0, e1 / a1, e2 / a2);
        V = sd * sd;
    }
    A.Pout[p] = valid ? make_float4(c0 / a0, c1 / a1, c2 / a2, V) : make_float4(c0, c1, c2, -1.0f);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (A.flags & DN_HAS_NORMAL) {
        const float n0 = A.normal[p * 3], n1 = A.normal[p * 3 + 1], n2 = A.normal[p * 3 + 2];
        const float l2 = (n0 * n0 + n1 * n1) + n2 * n2;
        if (!(l2 < 1e-12f) && dn_finite(l2)) { const float l = sqrtf(l2); g.x = n0 / l; g.y = n1 / l; g.z = n2 / l; }
    }
    float2 sl = make_float2(0.0f, 0.0f);
    if (A.flags & DN_HAS_DEPTH) {
        const float z = A.depth[p];
        g.w = dn_finite(z) ? z : INFINITY;
        if (dn_finite(z)) {
            const float zl = x > 0 ? A.depth[p - 1] : INFINITY, zr = x + 1 < w ? A.depth[p + 1] : INFINITY;
            const float zd = y > 0 ? A.depth[p - A.width] : INFINITY, zu = y + 1 < h ? A.depth[p + A.width] : INFINITY;
            const bool l = dn_finite(zl), r = dn_finite(zr), d = dn_finite(zd), u = dn_finite(zu);
            sl.x = (l && r) ? (zr - zl) * 0.5f : (r ? zr - z : (l ? z - zl : 0.0f));
            sl.y = (d && u) ? (zu - zd) * 0.5f : (u ? zu - z : (d ? z - zd : 0.0f));
        }
    }
    A.G[p] = g; A.S[p] = sl;
}

// One pass for the pixel (x, y), both forms: tap(dx, dy, Pq, Gq) fetches the tap at (x + s dx, y + s dy), false = outside the image.
template <class Tap>
__device__ __forceinline__ void dn_level_pixel(const DnArgs &A, int x, int y, Tap tap) {
    const int w = (int)A.width, h = (int)A.height;
    const size_t p = (size_t)y * A.width + x;
    const float4 Pp = A.Pin[p];
    if (Pp.w < 0.0f) {            // invalid: passes through, and comes out as the colour it came in with
        if (A.flags & DN_LAST) { A.out[p * 3] = A.color[p * 3]; A.out[p * 3 + 1] = A.color[p * 3 + 1]; A.out[p * 3 + 2] = A.color[p * 3 + 2]; }
        else A.Pout[p] = Pp;
        return;
    }
    const float4 Gp = A.G[p];
    const float2 Sp = A.S[p];
    const float Yp = dn_lum(Pp.x, Pp.y, Pp.z);
    float den_l = 1.0f;
    if (A.flags & DN_HAS_STDERR) {       // V through (1 2 1; 2 4 2; 1 2 1) over the adjacent valid pixels
        float acc = 0.0f, ws = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const float v = A.Pin[(size_t)qy * A.width + qx].w;
                if (v < 0.0f) continue;
                const float kw = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
                acc += kw * v; ws += kw;
            }
        den_l = A.sigma_l * sqrtf(acc / ws) + 1e-6f;
    }
    const bool p_flat = Gp.x == 0.0f && Gp.y == 0.0f && Gp.z == 0.0f, p_far = Gp.w == INFINITY;
    float W = 0.0f, J0 = 0.0f, J1 = 0.0f, J2 = 0.0f, U = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const float ky = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float hk = (dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f)) * ky;
            float4 Pq = Pp, Gq = Gp;
            float wt = hk;
            if (dx != 0 || dy != 0) {
                if (!tap(dx, dy, Pq, Gq)) continue;
                if (Pq.w < 0.0f) continue;
                float wn = 1.0f, xz = 0.0f, xl = 0.0f;
                if (A.flags & DN_HAS_NORMAL) {
                    const bool q_flat = Gq.x == 0.0f && Gq.y == 0.0f && Gq.z == 0.0f;
                    if (!(p_flat && q_flat)) {          // (one without a normal: the dot product is 0)
                        wn = fmaxf(0.0f, (Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z);
                        for (uint32_t i = 0; i < A.normal_squarings; i++) wn = wn * wn;
                    }
                }
                if (A.flags & DN_HAS_DEPTH) {
                    const bool q_far = Gq.w == INFINITY;
                    if (p_far != q_far) continue;
                    if (!p_far) xz = fabsf(Gp.w - Gq.w) /
                        (A.sigma_z * (fabsf(Sp.x * (float)(A.s * dx) + Sp.y * (float)(A.s * dy)) + 0.001f * Gp.w));
                }
                if (A.flags & DN_HAS_STDERR) xl = fabsf(Yp - dn_lum(Pq.x, Pq.y, Pq.z)) / den_l;
                wt = ((hk * wn) * dn_falloff(xz)) * dn_falloff(xl);
            }
            W += wt; J0 += wt * Pq.x; J1 += wt * Pq.y; J2 += wt * Pq.z; U += (wt * wt) * Pq.w;
        }
    }
    const float i0 = J0 / W, i1 = J1 / W, i2 = J2 / W;
    if (A.flags & DN_LAST) {
        float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
        if (A.flags & DN_HAS_ALBEDO) {
            a0 = fmaxf(A.albedo[p * 3], A.albedo_floor); a1 = fmaxf(A.albedo[p * 3 + 1], A.albedo_floor);
            a2 = fmaxf(A.albedo[p * 3 + 2], A.albedo_floor);
        }
        A.out[p * 3] = i0 * a0; A.out[p * 3 + 1] = i1 * a1; A.out[p * 3 + 2] = i2 * a2;
    } else {
        A.Pout[p] = make_float4(i0, i1, i2, U / (W * W));
    }
}

// the plain form: one thread per pixel, every tap two 16-byte global loads.  The yardstick of the staged form, and the form of the
// levels where staging does not pay (or does not fit).
__global__ __launch_bounds__(DN_BLOCK) void denoise_level_plain_kernel(DnArgs A) {
    const int x = (int)(blockIdx.x * DN_SX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * DN_R + (threadIdx.x >> 6));
    const int w = (int)A.width, h = (int)A.height;
    if (x >= w || y >= h) return;
    dn_level_pixel(A, x, y, [&](int dx, int dy, float4 &Pq, float4 &Gq) {
        const int qx = x + A.s * dx, qy = y + A.s * dy;
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) return false;
        const size_t q = (size_t)qy * A.width + qx;
        Pq = A.Pin[q]; Gq = A.G[q];
        return true;
    });
}

// the staged form: a workgroup owns DN_SX contiguous x and the DN_R rows y0, y0 + s, .. of one residue class of y mod s, whose taps
// are each other's.  It stages the DN_R + 4 rows y0 - 2s .. y0 + (DN_R + 1)s of DN_SX + 4s pixels in LDS, coalesced (a slot outside the
// image is stored as an invalid pixel, which the tap loop skips like the plain form's bounds test), and serves the 25 taps from there:
// (DN_R + 4)(DN_SX + 4s) / (DN_R DN_SX) staged pixels per output instead of 24.  P and G are separate arrays, so a wave's 64 lanes read 64
// consecutive 16-byte slots: no bank conflict.  Dynamic LDS: dn_staged_lds_bytes(s).
__host__ __device__ constexpr uint32_t dn_staged_lds_bytes(int s) { return (uint32_t)((DN_R + 4) * (DN_SX + 4 * s) * 2 * 16); }
__global__ __launch_bounds__(DN_BLOCK) void denoise_level_staged_kernel(DnArgs A) {
    extern __shared__ float4 dn_lds[];
    const int w = (int)A.width, h = (int)A.height, s = A.s, cols = DN_SX + 4 * s, slots = (DN_R + 4) * cols;
    float4 *sP = dn_lds, *sG = dn_lds + slots;
    const int x0 = (int)blockIdx.x * DN_SX;
    const int y0 = (int)(blockIdx.y % (uint32_t)s) + s * (int)(blockIdx.y / (uint32_t)s) * DN_R;
    for (int i = (int)threadIdx.x; i < slots; i += DN_BLOCK) {
        const int j = i / cols, c = i - j * cols;
        const int qx = x0 - 2 * s + c, qy = y0 + (j - 2) * s;
        float4 P = make_float4(0.0f, 0.0f, 0.0f, -1.0f), G = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qx >= 0 && qx < w && qy >= 0 && qy < h) { const size_t q = (size_t)qy * A.width + qx; P = A.Pin[q]; G = A.G[q]; }
        sP[i] = P; sG[i] = G;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6);
    const int x = x0 + tx, y = y0 + k * s;
    if (x >= w || y >= h) return;
    dn_level_pixel(A, x, y, [&](int dx, int dy, float4 &Pq, float4 &Gq) {
        const int i = (k + 2 + dy) * cols + tx + 2 * s + s * dx;
        Pq = sP[i]; Gq = sG[i];
        return true;
    });
}

// vk_progress_stderr on the device: the same expression in double, in the host call's operation order (no contraction), per pixel of the
// partition; N and k are the tile's own where adaptive sampling froze it.
__global__ void progress_stderr_kernel(const long long *run, const double *m2, const uint32_t *tile_n, const uint32_t *tile_k, uint32_t done,
                                       uint32_t steps, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tile_rank,
                                       uint32_t tile_world, float *out) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)width * height) return;
    const uint32_t x = (uint32_t)(pix % width), y = (uint32_t)(pix / width);
    const uint32_t t = (y / TILE) * tiles_x + x / TILE;
    if (t % tile_world != tile_rank) return;
    const uint32_t slot = (t - tile_rank) / tile_world;
    const uint32_t tn = tile_n ? tile_n[slot] : 0u;
    const double N = (double)(tn ? tn : done), k = (double)(tn ? tile_k[slot] : steps);
    for (int c = 0; c < 3; c++) {
        const size_t i = pix * 3 + c;
        const double mean = (double)run[i] / (double)ACCUM_SCALE / N;
        const double v = (m2[i] - N * mean * mean) / ((k - 1.0) * N);
        out[i] = (float)sqrt(v > 0.0 ? v : 0.0);
    }
}

// ---- temporal accumulation (vk_temporal_accumulate): one pass, one thread per pixel, f32, unfused, in the order the header
// (include/vecchio_amd.h) writes down; tests/temporal_ref.py restates it in numpy and the results agree bit for bit.  The history is three
// float4 planes of width*height pixels each, so that a tap is three 16-byte loads:
//   H[pixel]      = (I_r, I_g, I_b, N)   accumulated demodulated colour and its history length; N = 0: an INVALID pixel, never a tap
//   H[n + pixel]  = (V_r, V_g, V_b, z)   its variance per component; the depth of the frame that wrote it, +inf = nothing hit
//   H[2n + pixel] = (n_x, n_y, n_z, -)   that frame's unit normal, (0,0,0) = no normal
// A frame reads Hin (what the previous frame wrote) and writes Hout.  A workgroup is DN_R rows of DN_SX pixels, one wave per row: under a
// small camera step a wave's taps fall in two or three contiguous rows of the history.  The cameras and the projection constants (q, fw,
// H'.H', V'.V') come as kernel arguments: wave-uniform, held in SGPRs.  pixels_with_history: one ballot and one vector atomic per wave.
constexpr uint32_t TA_HAS_STDERR = 1u, TA_HAS_ALBEDO = 2u, TA_HAS_HISTORY = 4u;
struct TaArgs {
    const float4 *Hin; float4 *Hout;
    const float *color, *stderr3, *albedo, *normal, *depth;
    float *out_color, *out_stderr3, *out_history;                   // (the last two may be null)
    unsigned long long *count;
    uint32_t width, height, flags;
    float max_history, depth_tol, normal_cos_min, albedo_floor;
    float o[3], llc[3], H[3], V[3];                                 // this frame's camera
    float po[3], pq[3], pw[3], pH[3], pV[3];                        // the previous frame's: o', q = llc' - o', w', H', V'
    float fw, HH, VV;                                               // -(q . w'), H' . H', V' . V'
};

__device__ __forceinline__ float ta_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(DN_BLOCK) void temporal_accumulate_kernel(TaArgs A) {
    const int x = (int)(blockIdx.x * DN_SX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * DN_R + (threadIdx.x >> 6));
    const int w = (int)A.width, h = (int)A.height;
    bool took = false;
    if (x < w && y < h) {
        const size_t n = (size_t)A.width * A.height, p = (size_t)y * A.width + x;
        const float c0 = A.color[p * 3], c1 = A.color[p * 3 + 1], c2 = A.color[p * 3 + 2];
        bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2);
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
        if (A.flags & TA_HAS_STDERR) {
            e0 = A.stderr3[p * 3]; e1 = A.stderr3[p * 3 + 1]; e2 = A.stderr3[p * 3 + 2];
            valid = valid && dn_finite(e0) && dn_finite(e1) && dn_finite(e2);
        }
        if (!valid) {                 // passes through, and is stored as a pixel that is never a tap
            A.out_color[p * 3] = c0; A.out_color[p * 3 + 1] = c1; A.out_color[p * 3 + 2] = c2;
            if (A.out_stderr3) { A.out_stderr3[p * 3] = e0; A.out_stderr3[p * 3 + 1] = e1; A.out_stderr3[p * 3 + 2] = e2; }
            if (A.out_history) A.out_history[p] = 0.0f;
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            A.Hout[p] = zero; A.Hout[n + p] = zero; A.Hout[2 * n + p] = zero;
        } else {
            float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
            if (A.flags & TA_HAS_ALBEDO) {
                a0 = fmaxf(A.albedo[p * 3], A.albedo_floor); a1 = fmaxf(A.albedo[p * 3 + 1], A.albedo_floor);
                a2 = fmaxf(A.albedo[p * 3 + 2], A.albedo_floor);
            }
            float I0 = c0 / a0, I1 = c1 / a1, I2 = c2 / a2;
            float V0 = 0.0f, V1 = 0.0f, V2 = 0.0f;
            if (A.flags & TA_HAS_STDERR) {
                const float s0 = e0 / a0, s1 = e1 / a1, s2 = e2 / a2;
                V0 = s0 * s0; V1 = s1 * s1; V2 = s2 * s2;
            }
            float n0 = A.normal[p * 3], n1 = A.normal[p * 3 + 1], n2 = A.normal[p * 3 + 2];
            const float l2 = ta_dot(n0, n1, n2, n0, n1, n2);
            const bool p_flat = !(!(l2 < 1e-12f) && dn_finite(l2));
            if (p_flat) { n0 = 0.0f; n1 = 0.0f; n2 = 0.0f; }
            else { const float l = sqrtf(l2); n0 = n0 / l; n1 = n1 / l; n2 = n2 / l; }
            float z = A.depth[p];
            if (!dn_finite(z)) z = INFINITY;
            float N = 1.0f;
            if (A.flags & TA_HAS_HISTORY) {
                const float s = ((float)x + 0.5f) / (float)(w - 1), t = ((float)y + 0.5f) / (float)(h - 1);
                const float d0 = ((A.llc[0] + A.H[0] * s) + A.V[0] * t) - A.o[0], d1 = ((A.llc[1] + A.H[1] * s) + A.V[1] * t) - A.o[1],
                            d2 = ((A.llc[2] + A.H[2] * s) + A.V[2] * t) - A.o[2];
                const bool miss = z == INFINITY;
                float g0 = d0, g1 = d1, g2 = d2, ze = 0.0f;            // e, then g
                if (!miss) {
                    const float r = z / sqrtf(ta_dot(d0, d1, d2, d0, d1, d2));
                    g0 = (A.o[0] + d0 * r) - A.po[0]; g1 = (A.o[1] + d1 * r) - A.po[1]; g2 = (A.o[2] + d2 * r) - A.po[2];
                    ze = sqrtf(ta_dot(g0, g1, g2, g0, g1, g2));
                }
                const float ew = -ta_dot(g0, g1, g2, A.pw[0], A.pw[1], A.pw[2]);
                if (ew > 0.0f) {
                    const float r = A.fw / ew;
                    g0 = g0 * r - A.pq[0]; g1 = g1 * r - A.pq[1]; g2 = g2 * r - A.pq[2];
                    const float px = (ta_dot(g0, g1, g2, A.pH[0], A.pH[1], A.pH[2]) / A.HH) * (float)(w - 1) - 0.5f;
                    const float py = (ta_dot(g0, g1, g2, A.pV[0], A.pV[1], A.pV[2]) / A.VV) * (float)(h - 1) - 0.5f;
                    if (px > -1.0f && px < (float)w && py > -1.0f && py < (float)h) {
                        const float xf = floorf(px), yf = floorf(py), fx = px - xf, fy = py - yf;
                        const int x0 = (int)xf, y0 = (int)yf;
                        float W = 0.0f, J0 = 0.0f, J1 = 0.0f, J2 = 0.0f, U0 = 0.0f, U1 = 0.0f, U2 = 0.0f, M = 0.0f;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                            const float b = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                            const size_t q = (size_t)qy * A.width + qx;
                            const float4 hi = A.Hin[q], hv = A.Hin[n + q], hn = A.Hin[2 * n + q];
                            if (!(hi.w > 0.0f)) continue;
                            if (miss ? !(hv.w == INFINITY) : !(fabsf(hv.w - ze) <= A.depth_tol * ze)) continue;
                            const bool q_flat = hn.x == 0.0f && hn.y == 0.0f && hn.z == 0.0f;
                            if (p_flat != q_flat) continue;
                            if (!p_flat && !(ta_dot(n0, n1, n2, hn.x, hn.y, hn.z) >= A.normal_cos_min)) continue;
                            W += b; J0 += b * hi.x; J1 += b * hi.y; J2 += b * hi.z;
                            U0 += b * hv.x; U1 += b * hv.y; U2 += b * hv.z; M += b * hi.w;
                        }
                        if (W >= 0.01f) {
                            took = true;
                            N = fminf(M / W + 1.0f, A.max_history);
                            const float alpha = 1.0f / N, k = 1.0f - alpha, kk = k * k, aa = alpha * alpha;
                            I0 = k * (J0 / W) + alpha * I0; I1 = k * (J1 / W) + alpha * I1; I2 = k * (J2 / W) + alpha * I2;
                            V0 = kk * (U0 / W) + aa * V0; V1 = kk * (U1 / W) + aa * V1; V2 = kk * (U2 / W) + aa * V2;
                        }
                    }
                }
            }
            A.out_color[p * 3] = I0 * a0; A.out_color[p * 3 + 1] = I1 * a1; A.out_color[p * 3 + 2] = I2 * a2;
            if (A.out_stderr3) {
                A.out_stderr3[p * 3] = sqrtf(V0) * a0; A.out_stderr3[p * 3 + 1] = sqrtf(V1) * a1; A.out_stderr3[p * 3 + 2] = sqrtf(V2) * a2;
            }
            if (A.out_history) A.out_history[p] = N;
            A.Hout[p] = make_float4(I0, I1, I2, N); A.Hout[n + p] = make_float4(V0, V1, V2, z); A.Hout[2 * n + p] = make_float4(n0, n1, n2, 0.0f);
        }
    }
    const unsigned long long m = __ballot(took);
    if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(A.count, (unsigned long long)__popcll(m));
}

// ---- radiance queries (vk_trace_radiance): ray_color for rays read from memory.  render_kernel's shape — a persistent kernel, the
// wave-level phase scheduler (BOX / PRIM / SHADE + REFILL), idle lanes refilled by ballot + prefix popcount, cold path state parked in
// the wave's LDS block, finished samples summed in 64-bit fixed point — around a different REFILL: a work unit is (64 consecutive rays,
// a chunk of samples), item k of it is ray slot k & 63, sample s0 + (k >> 6).  A refilled lane loads its vk_ray as two 16-byte loads,
// seeds its stream from the ray's index (or from keys[i], the test hook) and starts its first segment with the ray's tmax as the
// closest distance so far.  A unit's sums collect in the wave's 64 x 3 LDS accumulators and reach the launch's sums (accum, one triple
// per ray) when the wave pulls its next unit; radiance_resolve_kernel divides.  With `samples` set every sample's 16 bytes are stored
// instead (the per-sample hook).  The scene is walked from global memory on the ray queries' tree view (vk_api.hip aov_view): no
// rebuilt form, no requeue, no probe build; a new kernel, so that no instance of render_kernel changes.
struct RadianceKey { uint64_t seed; uint32_t pixel, sample, ctr, _pad; };      // vk_debug_stream_key (vecchio_amd_debug.h)
struct RadianceArgs {
    DScene S;                // a tree view (vk_api.hip aov_view)
    RenderConsts C;          // seed, spp = samples_per_ray, max_depth, integrator, background; no camera, no image size
    const float4 *rays;      // vk_ray[n_rays]
    const RadianceKey *keys; // [n_rays] or null = the public rule
    long long *accum;        // [n_rays * 3] fixed-point sums, or null (the per-sample hook)
    float4 *samples;         // [n_rays * spp] (rgb, final counter) or null
    uint32_t *counter;       // work-unit counter
    unsigned long long *clamped;
    float accum_clamp;
    uint64_t first_index;
    uint32_t n_rays, first_sample, n_chunks, shade_defer, prim_weight;
    float4 *dirs;            // gather_kernel's per-sample hook: [n_rays * spp] (the drawn direction, 0) or null.  Last, so that every
                             // other field keeps the offset radiance_kernel was built with
};
typedef const __attribute__((address_space(4))) RadianceArgs *RArgsC;
__device__ __forceinline__ RArgsC rargs_fresh() {       // (see kargs_fresh)
    RArgsC p = (RArgsC)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#define RARG(p, field) (*(const decltype(RadianceArgs::field) *)&((p)->field))
constexpr int RAD_BLOCK = 256;       // 4 waves per workgroup
enum : int { RS_BLOCK = 0, RS_S0 = 1, RS_TOTAL = 2, RS_NEXT = 3 };      // the wave state: the unit being handed out (cf. WS_*)

// adds the wave's LDS sums of ray block `blk` (lane = ray slot) to the launch's accumulators and clears them
__device__ __forceinline__ void flush_ray_sums(unsigned long long *sums, long long *accum, uint32_t blk, uint32_t lane, uint32_t n_rays) {
    const uint32_t r = blk * 64u + lane;
    if (!accum || blk == 0xFFFFFFFFu || r >= n_rays) return;
    unsigned long long *a = reinterpret_cast<unsigned long long *>(accum) + (size_t)r * 3;
    for (int c = 0; c < 3; c++) {
        unsigned long long v = sums[lane * 3 + c];
        if (v) { atomicAdd(a + c, v); sums[lane * 3 + c] = 0ull; }
    }
}

// the three path queries: what the refill reads a record as (radiance_phase)
enum : int { QM_RAY = 0, QM_GATHER = 1, QM_PROBE = 2 };
// probe_kernel's work unit is (8 consecutive probes, a chunk of samples): 27 sums a probe, 8 x 27 x u64 = 1 728 bytes of LDS a wave
constexpr uint32_t PROBE_SLOTS = 8u, PROBE_VALUES = 27u;
template <int MODE> constexpr uint32_t query_sum_floats() { return MODE == QM_PROBE ? PROBE_SLOTS * PROBE_VALUES * 2u : 64u * 3u * 2u; }
// per-wave LDS block of a path-query kernel: wave_block_floats with the kernel's own sums
template <uint32_t F, int MODE> constexpr uint32_t query_block_floats() {
    return 64u * (uint32_t)ncold<F>() + query_sum_floats<MODE>() + (uint32_t)WAVE_STATE_WORDS; }

// adds the wave's LDS sums of probe block `blk` (8 probes x 27 values, contiguous as the launch's are) to the launch's accumulators and
// clears them: 216 values over the 64 lanes
__device__ __forceinline__ void flush_probe_sums(unsigned long long *sums, long long *accum, uint32_t blk, uint32_t lane, uint32_t n_probes) {
    if (!accum || blk == 0xFFFFFFFFu) return;
    unsigned long long *a = reinterpret_cast<unsigned long long *>(accum) + (size_t)blk * (PROBE_SLOTS * PROBE_VALUES);
    for (uint32_t j = lane; j < PROBE_SLOTS * PROBE_VALUES; j += 64u) {
        if (blk * PROBE_SLOTS + j / PROBE_VALUES >= n_probes) break;          // slots behind the batch's last probe
        unsigned long long v = sums[j];
        if (v) { atomicAdd(a + j, v); sums[j] = 0ull; }
    }
}

// a finished, finite sample `rgb` of probe r (counted from the launch's first), sample index smp: the direction drawn again from the
// stream's beginning, the nine basis values, and the 27 products in fixed point — converted and clamped as a radiance component is, the
// sample counted once if a product was clamped — into the wave's LDS sums (the block being handed out) or the launch's (a straggler).
// A non-finite direction (random_in_unit_sphere gave zero) drops the sample.
__device__ __forceinline__ void probe_accumulate(RArgsC P, const RenderConsts &C, long long *acc, unsigned long long *sums,
                                                 const uint32_t *wstate, uint32_t r, uint32_t smp, V3 rgb) {
    Rng g = radiance_rng(C.seed, RARG(P, first_index) + r, smp);
    const V3 u = probe_direction(g);
    if (!(isfinite(u.x) && isfinite(u.y) && isfinite(u.z))) return;
    float Y[9];
    sh9(u, Y);
    const float clampv = RARG(P, accum_clamp);
    const float rgbv[3] = {rgb.x, rgb.y, rgb.z};
    float big = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) big = fmaxf(big, fabsf(Y[k] * rgbv[c]));
    }
    const bool small = big <= ACCUM_SMALL;
    if (!small && big > clampv) atomicAdd(RARG(P, clamped), 1ull);     // (rare)
    auto add = [&](unsigned long long *t) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float v = Y[k] * rgbv[c];
                const unsigned long long f = (unsigned long long)(small ? to_fixed_small(v) : to_fixed(v, clampv));
                if (f) atomicAdd(t + (k * 3 + c), f);
            }
        }
    };
    if ((r / PROBE_SLOTS) == __builtin_amdgcn_readfirstlane(wstate[RS_BLOCK])) add(sums + (r % PROBE_SLOTS) * PROBE_VALUES);
    else add(reinterpret_cast<unsigned long long *>(acc) + (size_t)r * PROBE_VALUES);
}

// the SHADE + REFILL phase (cf. shade_refill_body).  Leaves `fresh` lanes with a new ray parked in L.wo / L.wd / L.time; t0 / walk are
// what its first segment starts with (radiance_start_core; +inf / true for a path that continues).  QM_GATHER (gather_kernel,
// vk_trace_irradiance): the record read is a point — origin p, direction the normal n — and the ray is made here: the lane draws
// irradiance_direction from the sample's stream, parks (p, d, time) and hands radiance_start_core the stream behind the draw.  QM_PROBE
// (probe_kernel, vk_trace_probes): the record is a probe — origin p, direction not read — and the lane draws probe_direction; a finished
// sample draws it AGAIN from the stream's beginning (no path state holds it) and adds its 27 products sh9 x rgb (probe_accumulate).
// SLOTS: the records of a work unit, 64 (lane = slot at the flush) or, for the probes' 27 sums a record, 8.
template <uint32_t F, int MODE = QM_RAY, uint32_t SLOTS = 64u>
__device__ __forceinline__ void radiance_phase(Lane &L, bool is_shade, bool &active, bool &need, bool &fresh, bool &touched, float &t0,
                                               bool &walk, RArgsC P, float *cold, unsigned long long *sums, uint32_t *wstate, uint32_t lane) {
    RenderConsts C = RARG(P, C);
    DScene S = RARG(P, S);
    GlobalMem M = make_mem<F, false>(S, 0u);
    fresh = false; t0 = INFINITY; walk = true;
    const PreTurb pre_turb = cooperative_turb<F, GlobalMem>(L, S, M, is_shade, lane);
    touched = is_shade;
    if (is_shade) {
        cold_load_path<F>(cold, lane, L);
        V3 no, nd; float nt;
        bool cont = shade_core<F, GlobalMem>(L, S, M, C, no, nd, nt, pre_turb, no_pre_ball());
        if (cont) { L.wo = no; L.wd = nd; L.time = nt; fresh = true; }
        else {
            const uint32_t r = __float_as_uint(cold[CF_XY * 64 + lane]);       // the ray, counted from the launch's first
            float4 *dbg = RARG(P, samples);
            if (dbg) dbg[(size_t)r * C.spp + (__float_as_uint(cold[CF_SAMPLE * 64 + lane]) - RARG(P, first_sample))] =
                make_float4(L.acc.x, L.acc.y, L.acc.z, __uint_as_float(L.rng.ctr));
            long long *acc = RARG(P, accum);
            if (MODE == QM_PROBE) {
                if (acc && isfinite(L.acc.x) && isfinite(L.acc.y) && isfinite(L.acc.z))
                    probe_accumulate(P, C, acc, sums, wstate, r, __float_as_uint(cold[CF_SAMPLE * 64 + lane]), L.acc);
            } else
            if (acc && isfinite(L.acc.x) && isfinite(L.acc.y) && isfinite(L.acc.z)) {   // main.rs:192-194; c += color (main.rs:193)
                const float clampv = RARG(P, accum_clamp);
                const float big = fmaxf(fmaxf(fabsf(L.acc.x), fabsf(L.acc.y)), fabsf(L.acc.z));
                unsigned long long fx, fy, fz;
                if (big <= ACCUM_SMALL) {
                    fx = (unsigned long long)to_fixed_small(L.acc.x); fy = (unsigned long long)to_fixed_small(L.acc.y);
                    fz = (unsigned long long)to_fixed_small(L.acc.z);
                } else {
                    if (big > clampv) atomicAdd(RARG(P, clamped), 1ull);     // (rare)
                    fx = (unsigned long long)to_fixed(L.acc.x, clampv); fy = (unsigned long long)to_fixed(L.acc.y, clampv);
                    fz = (unsigned long long)to_fixed(L.acc.z, clampv);
                }
                // a sample of the block the wave is handing out lands in the wave's LDS sums; a straggler of an earlier unit goes to
                // the launch's sums directly
                if ((r >> 6) == __builtin_amdgcn_readfirstlane(wstate[RS_BLOCK])) {
                    unsigned long long *t = sums + (r & 63u) * 3u;
                    atomicAdd(t + 0, fx); atomicAdd(t + 1, fy); atomicAdd(t + 2, fz);
                } else {
                    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc) + (size_t)r * 3;
                    atomicAdd(a + 0, fx); atomicAdd(a + 1, fy); atomicAdd(a + 2, fz);
                }
            }
            active = false;
            need = true;
        }
    }
    // ---- hand out (ray, sample) items of the wave's current unit to the lanes without a path; pull the next unit when it is used up
    for (;;) {
        unsigned long long need_mask = __builtin_amdgcn_ballot_w64(need);
        if (!need_mask) break;
        uint4 ws = *reinterpret_cast<const uint4 *>(wstate);
        uint32_t blk = __builtin_amdgcn_readfirstlane(ws.x), s0 = __builtin_amdgcn_readfirstlane(ws.y);
        uint32_t total = __builtin_amdgcn_readfirstlane(ws.z), next = __builtin_amdgcn_readfirstlane(ws.w);
        const uint32_t n_rays = RARG(P, n_rays);
        if (next >= total) {
            uint32_t unit = 0;
            if (lane == 0) unit = atomicAdd(RARG(P, counter), 1u);
            unit = __builtin_amdgcn_readfirstlane(unit);
            const uint32_t n_chunks = RARG(P, n_chunks);
            // (the host keeps blocks x chunks below 2^31 and a chunk below 2^20 samples)
            if (unit >= ((n_rays + (SLOTS - 1u)) / SLOTS) * n_chunks) { need = false; break; }
            // the finished unit's sums so far
            if (MODE == QM_PROBE) flush_probe_sums(sums, RARG(P, accum), blk, lane, n_rays);
            else flush_ray_sums(sums, RARG(P, accum), blk, lane, n_rays);
            const uint32_t chunk = unit % n_chunks;
            blk = unit / n_chunks;
            s0 = (uint32_t)(((uint64_t)C.spp * chunk) / n_chunks);
            const uint32_t s1 = (uint32_t)(((uint64_t)C.spp * (chunk + 1)) / n_chunks);
            next = 0u; total = SLOTS * (s1 - s0);
            s0 += RARG(P, first_sample);
            if (lane == 0) { wstate[RS_BLOCK] = blk; wstate[RS_S0] = s0; wstate[RS_TOTAL] = total; }
        }
        const uint32_t k = next + (uint32_t)__popcll(need_mask & ((1ull << lane) - 1ull));
        if (need && k < total) {
            const uint32_t r = blk * SLOTS + (k % SLOTS), smp = s0 + k / SLOTS;
            if (r < n_rays) {                  // slots behind the batch's last ray are skipped: the lane asks again
                cold[CF_XY * 64 + lane] = __uint_as_float(r);
                cold[CF_SAMPLE * 64 + lane] = __uint_as_float(smp);
                const float4 *rays = RARG(P, rays);
                const float4 r0 = rays[(size_t)r * 2u], r1 = rays[(size_t)r * 2u + 1u];
                const RadianceKey *keys = RARG(P, keys);
                Rng g;
                if (keys) {
                    const RadianceKey kk = keys[r];
                    g = vk::rng_for_sample(kk.seed, kk.pixel, kk.sample + (smp - RARG(P, first_sample)));
                    g.ctr = kk.ctr;
                } else {
                    g = radiance_rng(C.seed, RARG(P, first_index) + r, smp);
                }
                V3 dir = v3(r1.x, r1.y, r1.z);
                if (MODE != QM_RAY) {
                    dir = MODE == QM_PROBE ? probe_direction(g) : irradiance_direction(g, dir);
                    float4 *dd = RARG(P, dirs);
                    if (dd) dd[(size_t)r * C.spp + (smp - RARG(P, first_sample))] = make_float4(dir.x, dir.y, dir.z, 0.0f);
                }
                radiance_start_core(L, g, r0.w, t0, walk);
                L.wo = v3(r0.x, r0.y, r0.z); L.wd = dir; L.time = r1.w;
                fresh = true;
                active = true;
                need = false;
                touched = true;
            }
        }
        const uint32_t taken = (uint32_t)__popcll(need_mask);
        if (lane == 0) wstate[RS_NEXT] = next + taken < total ? next + taken : total;
    }
}

// the persistent loop of the three path-query kernels (radiance_kernel, gather_kernel, probe_kernel): they differ in the refill's
// ray-making step and, probe_kernel, in what a finished sample adds: 27 sums for each of a unit's 8 probes instead of 3 for each of 64 rays
template <uint32_t F, int MODE>
__device__ __forceinline__ void path_query_waves() {
    constexpr uint32_t SLOTS = MODE == QM_PROBE ? PROBE_SLOTS : 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    using Mem = GlobalMem;
    // ---- LDS layout: per wave [cold lane state | block sums: 64 x 3 x u64 (probe_kernel: 8 x 27 x u64) | wave state]
    float *cold = reinterpret_cast<float *>(smem) + wave * query_block_floats<F, MODE>();
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(cold + 64 * ncold<F>());
    uint32_t *wstate = reinterpret_cast<uint32_t *>(cold + 64 * ncold<F>() + query_sum_floats<MODE>());
    // the wave has no unit yet: the first SHADE + REFILL phase pulls one
    if (MODE == QM_PROBE) { for (uint32_t j = lane; j < PROBE_SLOTS * PROBE_VALUES; j += 64u) sums[j] = 0ull; }
    else { sums[lane * 3 + 0] = 0ull; sums[lane * 3 + 1] = 0ull; sums[lane * 3 + 2] = 0ull; }
    if (lane == 0) { wstate[RS_BLOCK] = 0xFFFFFFFFu; wstate[RS_NEXT] = 0u; wstate[RS_TOTAL] = 0u; }

    Lane L;
    __builtin_memset(&L, 0, sizeof(L));
    L.cur_inst = -1; L.cell = GRID_DONE;
    bool need = true;          // lane has no path and wants an item (false once the launch's units are all handed out)
    bool active = false;       // lane holds a live path
    uint32_t shade_defer, prim_weight;
    { RArgsC U = rargs_fresh(); shade_defer = RARG(U, shade_defer); prim_weight = RARG(U, prim_weight); }
    unsigned long long m_act = 0ull, m_need = ~0ull;
    // the scheduler of render_kernel (which see): the wave runs the code of the most populated state with the lanes in it
    for (;;) {
        const bool HAS_HEAVY = (F & (VKF_LIST | VKF_MEDIUM | VKF_INSTANCE | VKF_BOX)) != 0;
        const unsigned long long m_pend0 = __builtin_amdgcn_uicmp(L.pend, 0u, 33 /* ne */) & m_act;
        unsigned long long m_trav = __builtin_amdgcn_uicmp(L.i, L.end, 36 /* ult */);
        if (F & VKF_INSTANCE) m_trav |= __builtin_amdgcn_sicmp(L.cur_inst, 0, 39 /* sge */);
        const unsigned long long m_heavy = HAS_HEAVY ? (heavy_mask<F>(L.pend) & m_pend0) : 0ull;
        const unsigned long long m_light = m_pend0 & ~m_heavy;
        const unsigned long long m_shade = m_act & ~m_pend0 & ~m_trav;
        const uint32_t n_box = (uint32_t)__builtin_popcountll(m_act & ~m_pend0 & m_trav);
        const uint32_t n_heavy = (uint32_t)__builtin_popcountll(m_heavy), n_light = (uint32_t)__builtin_popcountll(m_light);
        const uint32_t n_prim = n_heavy > n_light ? n_heavy : n_light;
        const uint32_t n_sn = (uint32_t)__builtin_popcountll(m_shade | m_need);
        if ((n_box | n_prim | n_sn) == 0) break;
        if (n_box >= n_prim * prim_weight && n_box * shade_defer >= n_sn) {
            // ---- BOX: UNROLL steps under a shrinking EXEC mask per exit test, while box lanes are the plurality
            RArgsC P = rargs_fresh();
            DScene S = RARG(P, S);
            Mem M = make_mem<F, false>(S, 0u);
            const uint32_t live = n_box + n_heavy + n_light + n_sn;
            constexpr bool SPHERES = (F & ~(uint32_t)VKF_INTEG_PDF) == 0u;
            constexpr int UNROLL = ((F & VKF_ALL_SCENE) == VKF_ALL_SCENE) ? BOX_UNROLL + 1 : (SPHERES ? VK_GLOBAL_SPHERE_UNROLL : VK_CORNELL_UNROLL);
            unsigned long long m_pend, m_lt, m_inst = 0ull;
            auto masks = [&]() {
                m_pend = __builtin_amdgcn_uicmp(L.pend, 0u, 33 /* ne */);
                m_lt = __builtin_amdgcn_uicmp(L.i, range_end<F, Mem>(L, S), 36 /* ult */);
                if (F & VKF_INSTANCE) m_inst = __builtin_amdgcn_sicmp(L.cur_inst, 0, 39 /* sge */);
            };
            masks();
            for (;;) {
                if (F & VKF_INSTANCE) {     // end of an instance's item range: back to the parent space (rare)
                    const unsigned long long m_leave = m_act & ~m_pend & ~m_lt & m_inst;
                    if (m_leave != 0ull) {
                        if (__builtin_amdgcn_inverse_ballot_w64(m_leave)) { cold_load_world_ray<F>(cold, lane, L);
                            leave_instance<F, Mem>(L, S); }
                        masks();
                    }
                }
                const bool go = __builtin_amdgcn_inverse_ballot_w64(m_act & ~m_pend & m_lt);
                box_steps<F, Mem, UNROLL>(L, S, M, go);
                masks();
                const unsigned long long m_prim = m_pend & m_act, m_box = (m_lt | m_inst) & ~m_pend & m_act;
                const uint32_t nb = (uint32_t)__builtin_popcountll(m_box), np = (uint32_t)__builtin_popcountll(m_prim);
                const uint32_t ns = live - nb - np;
                const int keep1 = (int)nb - (int)(np * prim_weight > 1u ? np * prim_weight : 1u), keep2 = (int)(nb * shade_defer) - (int)ns;
                if ((keep1 | keep2) < 0) {
                    // a LIGHT primitive test runs right here and the loop keeps stepping (see render_kernel)
                    const unsigned long long m_lt2 = HAS_HEAVY ? (m_prim & ~heavy_mask<F>(L.pend)) : m_prim;
                    const uint32_t nl = (uint32_t)__builtin_popcountll(m_lt2);
                    if ((((int)nl - 1) | ((int)(2u * nl) - (int)np) | ((int)(nl * shade_defer) - (int)ns)) >= 0) {
                        if (__builtin_amdgcn_inverse_ballot_w64(m_lt2)) prim_step<F, Mem>(L, S, M);
                        masks();
                        continue;
                    }
                    break;
                }
            }
        } else if (n_prim * shade_defer >= n_sn) {
            // ---- PRIM: intersect / enter the pending object
            RArgsC P = rargs_fresh();
            DScene S = RARG(P, S);
            Mem M = make_mem<F, false>(S, 0u);
            if (__builtin_amdgcn_inverse_ballot_w64(n_heavy > n_light ? m_heavy : m_light)) {
                if (F & VKF_MEDIUM) {    // ConstantMedium::hit draws inside traversal (hittable.rs:473)
                    L.rng.key = (uint64_t)__float_as_uint(cold[CF_KEY * 64 + lane]) |
                                ((uint64_t)__float_as_uint(cold[(CF_KEY + 1) * 64 + lane]) << 32);
                    L.rng.ctr = __float_as_uint(cold[CF_CTR * 64 + lane]);
                }
                prim_step<F, Mem>(L, S, M);
                if (F & VKF_MEDIUM) cold[CF_CTR * 64 + lane] = __uint_as_float(L.rng.ctr);
            }
        } else {
            // ---- SHADE + REFILL; one begin_segment for both kinds of new ray
            const bool is_shade = __builtin_amdgcn_inverse_ballot_w64(m_shade);
            bool touched = false, fresh = false, walk = true;
            float t0 = INFINITY;
            radiance_phase<F, MODE, SLOTS>(L, is_shade, active, need, fresh, touched, t0, walk, rargs_fresh(), cold, sums, wstate, lane);
            if (fresh) {
                RArgsC P = rargs_fresh();
                DScene S = RARG(P, S);
                begin_segment<Mem::ISHIFT, fused_box<F, Mem>(), spheres_only<F>()>(L, S, L.wo, L.wd, L.time, false, t0);
                if (!walk) radiance_skip_walk(L);
            }
            if (active && touched) cold_store_path<F>(cold, lane, L);
            m_act = __builtin_amdgcn_ballot_w64(active); m_need = __builtin_amdgcn_ballot_w64(need);
        }
    }
    {   // the last unit's sums
        RArgsC P = rargs_fresh();
        if (MODE == QM_PROBE) flush_probe_sums(sums, RARG(P, accum), __builtin_amdgcn_readfirstlane(wstate[RS_BLOCK]), lane, RARG(P, n_rays));
        else flush_ray_sums(sums, RARG(P, accum), __builtin_amdgcn_readfirstlane(wstate[RS_BLOCK]), lane, RARG(P, n_rays));
    }
}

template <uint32_t F, int MINW>
__global__ __launch_bounds__(RAD_BLOCK, MINW) void radiance_kernel(RadianceArgs A_byval) {
    (void)A_byval;
    path_query_waves<F, QM_RAY>();
}

// ---- irradiance queries (vk_trace_irradiance): radiance_kernel around a refill that reads (point, normal) records and draws each
// sample's cosine-weighted direction on the device (radiance_phase<F, true>).  No per-path state is added: the normal is read again at
// every refill, as the ray is.  The arguments are radiance_kernel's (rays = the points, keys = null).
template <uint32_t F, int MINW>
__global__ __launch_bounds__(RAD_BLOCK, MINW) void gather_kernel(RadianceArgs A_byval) {
    (void)A_byval;
    path_query_waves<F, QM_GATHER>();
}

// ---- probe queries (vk_trace_probes): radiance_kernel around a refill that draws each sample's uniform direction on the device
// (radiance_phase<F, QM_PROBE, 8>) and a finish that projects the sample onto nine spherical-harmonic basis functions.  No per-path state
// is added: the finish draws the direction again from the sample's (index, sample).  The arguments are radiance_kernel's (rays = the
// probes, keys = null, accum = 27 sums a probe).
template <uint32_t F, int MINW>
__global__ __launch_bounds__(RAD_BLOCK, MINW) void probe_kernel(RadianceArgs A_byval) {
    (void)A_byval;
    path_query_waves<F, QM_PROBE>();
}

// ray mean = fixed-point sum / samples_per_ray (resolve_kernel's arithmetic)
__global__ void radiance_resolve_kernel(const long long *accum, float *out, uint32_t n_values, uint32_t spp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    const float inv_scale = 1.0f / ACCUM_SCALE;
    out[i] = ((float)accum[i] * inv_scale) / (float)spp;
}

// ---- shade queries (vk_shade_hits): vk_trace.h shade_hit for (ray, hit, path state) items read from memory, one item per lane, 64
// consecutive items per wave.  A lane reads its vk_ray, vk_hit and vk_path_state as two, four and three 16-byte loads and writes its
// vk_shaded as six 16-byte stores.  No walk, no LDS, no atomics: item i's result depends on (scene, params, item i) alone.  Perlin noise
// and the unit ball's rejection loop run inside the lane (no_pre_turb, no_pre_ball): the wave-cooperative forms of the path kernels
// give the same values by construction.  Two instances: every scene feature, with and without VKF_INTEG_PDF — nothing here is a
// traversal whose registers a narrower variant would save, and the material table is read by material index for every scene.
struct ShadeArgs {
    DScene S;                // a tree view (vk_api.hip aov_view); only its material, texture, light and primitive tables are read
    RenderConsts C;          // max_depth, integrator, background
    const float4 *rays;      // vk_ray[n]
    const uint4 *hits;       // vk_hit[n]
    const uint4 *states;     // vk_path_state[n]
    uint4 *out;              // vk_shaded[n]
    uint64_t n;
    uint32_t n_materials;    // the description's: the bound a caller's material index is checked against
};
template <uint32_t F>
__global__ __launch_bounds__(AOV_BLOCK) void shade_hits_kernel(ShadeArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * AOV_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    uint32_t ray[8], hit[16], st[12], w[24];
    {
        const float4 r0 = A.rays[i * 2u], r1 = A.rays[i * 2u + 1u];
        ray[0] = __float_as_uint(r0.x); ray[1] = __float_as_uint(r0.y); ray[2] = __float_as_uint(r0.z); ray[3] = __float_as_uint(r0.w);
        ray[4] = __float_as_uint(r1.x); ray[5] = __float_as_uint(r1.y); ray[6] = __float_as_uint(r1.z); ray[7] = __float_as_uint(r1.w);
        const uint4 *h = A.hits + i * 4u, *s = A.states + i * 3u;
#pragma unroll
        for (int k = 0; k < 4; k++) { const uint4 v = h[k]; hit[k * 4] = v.x; hit[k * 4 + 1] = v.y; hit[k * 4 + 2] = v.z; hit[k * 4 + 3] = v.w; }
#pragma unroll
        for (int k = 0; k < 3; k++) { const uint4 v = s[k]; st[k * 4] = v.x; st[k * 4 + 1] = v.y; st[k * 4 + 2] = v.z; st[k * 4 + 3] = v.w; }
    }
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    shade_hit<F, GlobalMem>(A.S, M, A.C, A.n_materials, ray, hit, st, w);
    uint4 *out = A.out + i * 6u;
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = make_uint4(w[k * 4], w[k * 4 + 1], w[k * 4 + 2], w[k * 4 + 3]);
}

// ---- path batches (vk_paths_*): a bounce is trace_paths_kernel, shade_hits_kernel and the compaction's three launches, all on buffers
// the handle owns.
// trace_paths_kernel: trace_rays_kernel's shape and its two variants, with vk_trace.h trace_path in place of trace_ray: a ConstantMedium
// draws from the PATH's stream — rng_for_sample(state.seed, state.pixel, state.sample) standing at state.counter — and the counter the
// walk leaves is stored back into the lane's own state.  The sphere-only variant can draw nothing and does not touch the states.
struct TracePathsArgs {
    DScene S;                // a tree view (vk_api.hip aov_view)
    DProvenance P;
    const float4 *rays;      // vk_ray[n]
    uint4 *states;           // vk_path_state[n]: the counter (word 7) is rewritten when F has VKF_MEDIUM
    uint4 *hits;             // vk_hit[n]
    uint64_t n;
};
template <uint32_t F>
__global__ __launch_bounds__(AOV_BLOCK) void trace_paths_kernel(TracePathsArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * AOV_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const float4 r0 = A.rays[i * 2u], r1 = A.rays[i * 2u + 1u];
    const uint32_t ray[8] = {__float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z), __float_as_uint(r0.w),
                             __float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), __float_as_uint(r1.w)};
    uint32_t st47[4] = {0u, 0u, 0u, 0u}, st811[4] = {0u, 0u, 0u, 0u};
    if (F & VKF_MEDIUM) {
        const uint4 a = A.states[i * 3u + 1u], b = A.states[i * 3u + 2u];
        st47[0] = a.x; st47[1] = a.y; st47[2] = a.z; st47[3] = a.w;
        st811[0] = b.x; st811[1] = b.y; st811[2] = b.z; st811[3] = b.w;
    }
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    uint32_t w[16];
    const uint32_t ctr = trace_path<F, GlobalMem>(A.S, M, A.P, ray, st47, st811, w);
    if (F & VKF_MEDIUM) A.states[i * 3u + 1u] = make_uint4(st47[0], st47[1], st47[2], ctr);
    uint4 *out = A.hits + i * 4u;
    out[0] = make_uint4(w[0], w[1], w[2], w[3]);
    out[1] = make_uint4(w[4], w[5], w[6], w[7]);
    out[2] = make_uint4(w[8], w[9], w[10], w[11]);
    out[3] = make_uint4(w[12], w[13], w[14], w[15]);
}

// The stable compaction of a bounce's vk_shaded[n] + ids[n]: item i survives when its status is VK_SHADE_SCATTERED; the survivors'
// next rays, states and ids go to rays[], states[] and ids_out[] in their order, a retired item's state and status to result_state[id]
// and result_status[id].  Three launches, joined by memory alone — no workgroup waits for another, no atomics, inputs and outputs
// distinct buffers — so the result does not depend on how the workgroups are scheduled:
//   paths_count_kernel   one item per lane, PATHS_T items per workgroup: the workgroup's items by status (ballots, joined through LDS)
//                        into wg_counts[status * n_wg + workgroup];
//   paths_scan_kernel    ONE workgroup: the exclusive prefix sums of the survivors' row into wg_offsets[], PATHS_SCAN_T workgroup counts
//                        per pass with the running total carried from pass to pass, and the five totals into counts[5];
//   paths_move_kernel    the count pass's shape: a survivor's slot is wg_offsets[workgroup] + the survivors of the workgroup's earlier
//                        waves (LDS) + its rank among its wave's survivors (mbcnt of the ballot's lower lanes); 16-byte accesses.
// A status above 4 is counted with VK_PATHS_CULLED (no kernel of the library writes one; the debug hook's caller may).
constexpr int PATHS_T = 256;             // items per workgroup of the count and move passes
constexpr int PATHS_SCAN_T = 256;        // workgroup counts per pass of the scan
constexpr uint32_t PATHS_STATUSES = 5u;  // VK_SHADE_MISS, SCATTERED, ENDED, BAD_HIT, VK_PATHS_CULLED
struct CompactArgs {
    const uint4 *items;         // vk_shaded[n]
    const uint32_t *ids;        // [n], each below n_ids
    uint64_t n, n_ids;
    uint4 *rays;                // vk_ray[survivors]
    uint4 *states;              // vk_path_state[survivors]
    uint32_t *ids_out;          // [survivors]
    uint4 *result_state;        // vk_path_state[n_ids]
    uint32_t *result_status;    // [n_ids]
    uint32_t *wg_counts;        // [PATHS_STATUSES][n_wg]
    uint32_t *wg_offsets;       // [n_wg]
    unsigned long long *counts; // [PATHS_STATUSES]
    uint32_t n_wg;
};
// The count pass's tally, for a lane of paths_count_kernel or roulette_count_kernel: the lane's status (below PATHS_STATUSES; `in` = the
// lane holds an item) is balloted status by status, the waves' counts meet in wc[] behind the ONE barrier, which every lane of the
// workgroup reaches, and the first five lanes write the workgroup's row entries.
__device__ __forceinline__ void tally_statuses(const CompactArgs &A, bool in, uint32_t status, uint32_t (&wc)[PATHS_T / 64][PATHS_STATUSES]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t s = 0; s < PATHS_STATUSES; s++) {
        const unsigned long long m = __ballot(in && status == s);
        if (lane == 0) wc[w][s] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < PATHS_STATUSES) {
        uint32_t t = 0;
        for (int k = 0; k < PATHS_T / 64; k++) t += wc[k][threadIdx.x];
        A.wg_counts[(size_t)threadIdx.x * A.n_wg + blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(PATHS_T) void paths_count_kernel(CompactArgs A) {
    __shared__ uint32_t wc[PATHS_T / 64][PATHS_STATUSES];
    const uint64_t i = (uint64_t)blockIdx.x * PATHS_T + threadIdx.x;
    const bool in = i < A.n;
    uint32_t status = 0u;
    if (in) { status = reinterpret_cast<const uint32_t *>(A.items + i * 6u)[20]; if (status >= PATHS_STATUSES) status = PATHS_STATUSES - 1u; }
    tally_statuses(A, in, status, wc);
}
// roulette_count_kernel: the count pass's second form, with the handle's termination rule (vk_roulette_set) in front of the tally.
// A record that is VK_SHADE_SCATTERED with state.depth >= first_depth is decided here, everything f32 and unfused:
//   m = fmaxf(fmaxf(thr.x, thr.y), thr.z), q = fminf(fmaxf(m, q_min), q_max)      (fmaxf drops a NaN: q lies in [q_min, q_max] whatever thr)
//       — as np.fmax does, for a signalling NaN too: v_max_f32 in IEEE mode answers one with a NaN, so the two are spelled as the
//       compare and select of max_drop_nan / min_drop_nan, whose answer never depends on a NaN's kind
//   u = draw number `depth` of the rule's own stream, rng_for_sample(state.seed ^ ROULETTE_SALT, state.pixel, state.sample): the
//       path's stream and state.counter are not touched
//   u < q: the path goes on with thr * (1.0f / q) — one IEEE division, three products: vk_paths_cull's thr * scale —, the first quarter
//       of its state rewritten; otherwise its status word becomes VK_PATHS_CULLED, the last quarter of the record rewritten, and the
//       state stays as the bounce left it.
// Both are 16-byte stores into the lane's own record, in front of the ballots, so that the scan and the move pass run unchanged on the
// rewritten records; the statuses are counted as they then stand.  No lane leaves before the tally.
constexpr uint64_t ROULETTE_SALT = 0x52D1E7A9C3B5F04Bull;
__device__ __forceinline__ float max_drop_nan(float a, float b) { return (a >= b || b != b) ? a : b; }
__device__ __forceinline__ float min_drop_nan(float a, float b) { return (a <= b || b != b) ? a : b; }
struct RouletteRule {
    uint32_t first_depth;
    float q_min, q_max;
};
__global__ __launch_bounds__(PATHS_T) void roulette_count_kernel(CompactArgs A, RouletteRule R) {
    __shared__ uint32_t wc[PATHS_T / 64][PATHS_STATUSES];
    const uint64_t i = (uint64_t)blockIdx.x * PATHS_T + threadIdx.x;
    const bool in = i < A.n;
    uint32_t status = 0u;
    if (in) {
        uint4 *item = const_cast<uint4 *>(A.items) + i * 6u;      // (the records are the handle's, or the hook's, own buffer)
        uint4 tail = item[5];
        status = tail.x;
        if (status == (uint32_t)VK_SHADE_SCATTERED) {
            uint4 s0 = item[2];                                   // thr, depth
            if (s0.w >= R.first_depth) {
                const uint4 s2 = item[4];                         // seed, pixel, sample
                const float tx = __uint_as_float(s0.x), ty = __uint_as_float(s0.y), tz = __uint_as_float(s0.z);
                const float q = min_drop_nan(max_drop_nan(max_drop_nan(max_drop_nan(tx, ty), tz), R.q_min), R.q_max);
                vk::Rng g = vk::rng_for_sample((((uint64_t)s2.y << 32) | (uint64_t)s2.x) ^ ROULETTE_SALT, s2.z, s2.w);
                g.ctr = s0.w - 1u;
                const float u = vk::gen_f32(g);
                if (u < q) {
                    const float k = 1.0f / q;
                    s0.x = __float_as_uint(tx * k); s0.y = __float_as_uint(ty * k); s0.z = __float_as_uint(tz * k);
                    item[2] = s0;
                } else {
                    status = tail.x = (uint32_t)VK_PATHS_CULLED;
                    item[5] = tail;
                }
            }
        }
        if (status >= PATHS_STATUSES) status = PATHS_STATUSES - 1u;
    }
    tally_statuses(A, in, status, wc);
}
__global__ __launch_bounds__(PATHS_SCAN_T) void paths_scan_kernel(CompactArgs A) {
    __shared__ uint32_t wt[PATHS_SCAN_T / 64];
    __shared__ unsigned long long tot[PATHS_SCAN_T / 64][PATHS_STATUSES];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long mine[PATHS_STATUSES] = {0ull, 0ull, 0ull, 0ull, 0ull};
    uint32_t running = 0u;                                       // survivors of the passes before this one
    for (uint32_t base = 0; base < A.n_wg; base += PATHS_SCAN_T) {
        const uint32_t b = base + threadIdx.x;
        const bool in = b < A.n_wg;
#pragma unroll
        for (uint32_t s = 0; s < PATHS_STATUSES; s++) mine[s] += in ? A.wg_counts[(size_t)s * A.n_wg + b] : 0u;
        const uint32_t v = in ? A.wg_counts[(size_t)VK_SHADE_SCATTERED * A.n_wg + b] : 0u;
        uint32_t incl = v;                                       // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63u) wt[w] = incl;
        __syncthreads();
        uint32_t before = running, all = 0u;
        for (uint32_t k = 0; k < PATHS_SCAN_T / 64; k++) { if (k < w) before += wt[k]; all += wt[k]; }
        if (in) A.wg_offsets[b] = before + incl - v;
        running += all;
        __syncthreads();                                         // (wt is rewritten by the next pass)
    }
#pragma unroll
    for (uint32_t s = 0; s < PATHS_STATUSES; s++) {              // the totals: a wave's sum by shuffles, the waves' through LDS
        unsigned long long t = mine[s];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
        if (lane == 0) tot[w][s] = t;
    }
    __syncthreads();
    if (threadIdx.x < PATHS_STATUSES) {
        unsigned long long t = 0ull;
        for (int k = 0; k < PATHS_SCAN_T / 64; k++) t += tot[k][threadIdx.x];
        A.counts[threadIdx.x] = t;
    }
}
// The move pass's survivor half, for a lane of paths_move_kernel or regen_move_kernel (A: either's arguments): item i's tail (status,
// lobe, pad; zeros outside [0, n)) is read and the SCATTERED lanes balloted; the waves' counts meet in wc[] behind the ONE barrier, which
// every lane of the workgroup reaches; a survivor's ray, state and id then go to its slot, 16-byte accesses.  (slot < n always: the
// offsets count these very items.)  What becomes of a retired item is the caller's.
struct Moved {
    bool go;                 // the lane holds a survivor
    uint4 tail;
};
template <class Args>
__device__ __forceinline__ Moved move_survivor(const Args &A, uint64_t i, uint32_t (&wc)[PATHS_T / 64]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint4 *item = A.items + i * 6u;
    Moved R{false, make_uint4(0u, 0u, 0u, 0u)};
    if (i < A.n) R.tail = item[5];
    R.go = i < A.n && R.tail.x == (uint32_t)VK_SHADE_SCATTERED;
    const unsigned long long m = __ballot(R.go);
    if (lane == 0) wc[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (R.go) {
        uint32_t slot = A.wg_offsets[blockIdx.x];
        for (uint32_t k = 0; k < w; k++) slot += wc[k];
        slot += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (slot < A.n) {
            uint4 *r = A.rays + (size_t)slot * 2u, *s = A.states + (size_t)slot * 3u;
            r[0] = item[0]; r[1] = item[1];
            s[0] = item[2]; s[1] = item[3]; s[2] = item[4];
            A.ids_out[slot] = A.ids[i];
        }
    }
    return R;
}
__global__ __launch_bounds__(PATHS_T) void paths_move_kernel(CompactArgs A) {
    __shared__ uint32_t wc[PATHS_T / 64];
    const uint64_t i = (uint64_t)blockIdx.x * PATHS_T + threadIdx.x;
    const Moved R = move_survivor(A, i, wc);
    if (i >= A.n || R.go) return;
    const uint32_t id = A.ids[i];
    if (id < A.n_ids) {
        const uint4 *item = A.items + i * 6u;
        uint4 *s = A.result_state + (size_t)id * 3u;
        s[0] = item[2]; s[1] = item[3]; s[2] = item[4];
        A.result_status[id] = R.tail.x;
    }
}
// ids[i] = i: the ids of a batch just begun
__global__ void paths_iota_kernel(uint32_t *ids, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = i;
}
// vk_paths_cull's marking pass: live item j as a vk_shaded record the compaction reads — next = its ray, state = its state (thr times
// scale[j], three f32 products, where scale is given and the path is kept), status VK_SHADE_SCATTERED for keep[j] != 0 and
// VK_PATHS_CULLED otherwise (the state then as it stands), lobe 0xFFFFFFFF.  The same compaction then runs: no second move pass.
__global__ __launch_bounds__(PATHS_T) void paths_cull_mark_kernel(const uint4 *rays, const uint4 *states, const uint8_t *keep, const float *scale,
                                                                  uint64_t n, uint4 *items) {
    const uint64_t i = (uint64_t)blockIdx.x * PATHS_T + threadIdx.x;
    if (i >= n) return;
    const bool kept = keep[i] != 0u;
    uint4 s0 = states[i * 3u];
    if (kept && scale) {
        const float k = scale[i];
        s0.x = __float_as_uint(__uint_as_float(s0.x) * k); s0.y = __float_as_uint(__uint_as_float(s0.y) * k);
        s0.z = __float_as_uint(__uint_as_float(s0.z) * k);
    }
    uint4 *out = items + i * 6u;
    out[0] = rays[i * 2u]; out[1] = rays[i * 2u + 1u];
    out[2] = s0; out[3] = states[i * 3u + 1u]; out[4] = states[i * 3u + 2u];
    out[5] = make_uint4(kept ? (uint32_t)VK_SHADE_SCATTERED : (uint32_t)VK_PATHS_CULLED, 0xFFFFFFFFu, 0u, 0u);
}

// ---- films (vk_film_*) and regeneration (vk_regen_*): the two ends of a frame made of path batches, on the device.  vk_film_emit fills
// a batch with film_emit_kernel and vk_film_deposit adds a finished one to the sums with film_deposit_kernel; a regenerating bounce is
// regen_emit_kernel (the top-up), trace_paths_kernel, shade_hits_kernel, the compaction's count and scan passes as they are, and
// regen_move_kernel.
constexpr int FILM_T = 256;
// the deposit's default form, measured (DESIGN.md "Film"): on C2's frame at 8 samples per pixel RUNS takes 0.79 of PLAIN's time, far
// beyond the spread of the repetitions; at 1 sample per pixel, where no two neighbours share a pixel, the two are level
constexpr bool FILM_DEPOSIT_RUNS = true;

// (EmitWindow and start_camera_path: vk_emit.h)
// film_emit_kernel: one lane per path of the window, path i in slot i: no iota launch.
struct FilmEmitArgs {
    RenderConsts C;          // the film's camera, frame and seed
    uint4 *rays;             // vk_ray[n]
    uint4 *states;           // vk_path_state[n]
    uint32_t *ids;           // [n]
    EmitWindow W;
    uint32_t n;
};
__global__ __launch_bounds__(FILM_T) void film_emit_kernel(FilmEmitArgs A) {
    const uint32_t i = blockIdx.x * FILM_T + threadIdx.x;
    if (i >= A.n) return;
    start_camera_path(A.C, A.W, i, (size_t)i, A.rays, A.states, A.ids);
}
// regen_emit_kernel: lane j < m starts path first + j of the window in slot slot0 + j.  first + m <= 2^32 - 1 (the host refuses a longer
// window), slot0 + m <= the batch's capacity.
struct RegenEmitArgs {
    RenderConsts C;          // the film's camera, frame and seed
    uint4 *rays;             // vk_ray[capacity]
    uint4 *states;           // vk_path_state[capacity]
    uint32_t *ids;           // [capacity]: the buffer that holds the live ids of this bounce
    EmitWindow W;
    uint32_t first, slot0, m;
};
__global__ __launch_bounds__(FILM_T) void regen_emit_kernel(RegenEmitArgs A) {
    const uint32_t j = blockIdx.x * FILM_T + threadIdx.x;
    if (j >= A.m) return;
    start_camera_path(A.C, A.W, A.first + j, (size_t)A.slot0 + j, A.rays, A.states, A.ids);
}

// The deposit of one lane's candidate — a path that has left its batch; cand = the lane holds one — from its status and the second and
// third quarter of its state (s1: acc, s2: pixel in .z).  A candidate retired as VK_SHADE_MISS, VK_SHADE_ENDED or VK_PATHS_CULLED goes
// to the pixel its STATE names: the render kernel's finite filter (main.rs:192-194) and its conversion (to_fixed_small at or below
// ACCUM_SMALL, else to_fixed with the film's clamp); the caller adds the three fixed values to the pixel's sums by 64-bit integer
// atomics where `deposit` is set.  A pixel outside the frame and every other status is skipped: `deposit` stays clear and nothing may be
// touched by that index.  The four counters — deposited, dropped, clamped, skipped (every candidate that is neither of the first two)
// — are ballots, one atomic per wave and non-zero counter: EVERY lane of the wave must call this, from uniform control flow.
struct Deposit {
    bool deposit;
    uint32_t pixel;
    unsigned long long fx, fy, fz;
};
__device__ __forceinline__ Deposit deposit_lane(bool cand, uint32_t status, uint4 s1, uint4 s2, uint32_t n_pixels, float accum_clamp,
                                                unsigned long long *counters) {
    const float ax = __uint_as_float(s1.x), ay = __uint_as_float(s1.y), az = __uint_as_float(s1.z);
    const bool retired = status == (uint32_t)VK_SHADE_MISS || status == (uint32_t)VK_SHADE_ENDED || status == (uint32_t)VK_PATHS_CULLED;
    const bool ours = cand && retired && s2.z < n_pixels;
    const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az);
    const float big = fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az));
    const bool large = big > ACCUM_SMALL;
    Deposit D{ours && finite, s2.z, 0ull, 0ull, 0ull};
    const unsigned long long m_dep = __ballot(D.deposit), m_drop = __ballot(ours && !finite);
    const unsigned long long m_clamp = __ballot(D.deposit && large && big > accum_clamp), m_skip = __ballot(cand && !ours);
    if ((threadIdx.x & 63u) == 0u) {
        if (m_dep) atomicAdd(counters + 0, (unsigned long long)__popcll(m_dep));
        if (m_drop) atomicAdd(counters + 1, (unsigned long long)__popcll(m_drop));
        if (m_clamp) atomicAdd(counters + 2, (unsigned long long)__popcll(m_clamp));
        if (m_skip) atomicAdd(counters + 3, (unsigned long long)__popcll(m_skip));
    }
    if (D.deposit) {
        if (!large) {
            D.fx = (unsigned long long)to_fixed_small(ax); D.fy = (unsigned long long)to_fixed_small(ay); D.fz = (unsigned long long)to_fixed_small(az);
        } else {
            D.fx = (unsigned long long)to_fixed(ax, accum_clamp); D.fy = (unsigned long long)to_fixed(ay, accum_clamp);
            D.fz = (unsigned long long)to_fixed(az, accum_clamp);
        }
    }
    return D;
}
__device__ __forceinline__ void deposit_add(unsigned long long *sums, const Deposit &D) {
    unsigned long long *a = sums + (size_t)D.pixel * 3u;
    atomicAdd(a + 0, D.fx); atomicAdd(a + 1, D.fy); atomicAdd(a + 2, D.fz);
}

// film_deposit_kernel<RUNS>: one lane per started id of a batch with nothing live; every id below n is a candidate, from its result.
//   RUNS = false (PLAIN): every depositing lane issues its three atomics.
//   RUNS = true: a wave's neighbouring lanes that deposit into the same pixel — after an emit, a pixel's n_samples paths — are summed
//     first, by a segmented suffix sum (six __shfl_down steps, a lane adds its neighbour at distance d while that one lies in its run),
//     and the head lane of a run issues the atomics for all of it.  Integer sums: both forms give the same bytes.
struct FilmDepositArgs {
    const uint4 *result_state;     // vk_path_state[n]
    const uint32_t *result_status; // [n]
    unsigned long long *sums;      // [n_pixels * 3]
    unsigned long long *counters;  // deposited, dropped, clamped, skipped
    uint32_t n, n_pixels;
    float accum_clamp;             // accum_clamp_for(the film's samples_per_pixel)
};
template <bool RUNS>
__global__ __launch_bounds__(FILM_T) void film_deposit_kernel(FilmDepositArgs A) {
    const uint32_t i = blockIdx.x * FILM_T + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = i < A.n;
    uint32_t status = (uint32_t)VK_SHADE_BAD_HIT;
    uint4 s1 = make_uint4(0u, 0u, 0u, 0u), s2 = s1;
    if (in) { status = A.result_status[i]; s1 = A.result_state[(size_t)i * 3u + 1u]; s2 = A.result_state[(size_t)i * 3u + 2u]; }
    Deposit D = deposit_lane(in, status, s1, s2, A.n_pixels, A.accum_clamp, A.counters);
    bool issue = D.deposit;
    if (RUNS) {
        const uint32_t key = D.deposit ? D.pixel : 0xFFFFFFFFu;             // (a depositing pixel is below n_pixels <= 2^26)
        const uint32_t prev = __shfl_up(key, 1, 64);
        const unsigned long long heads = __ballot(lane == 0u || prev != key);
        const unsigned long long above = heads & ~(((2ull << lane) - 1ull));     // the heads behind this lane (lane 63: none)
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;    // one past the lane's run
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const unsigned long long vx = __shfl_down(D.fx, d, 64), vy = __shfl_down(D.fy, d, 64), vz = __shfl_down(D.fz, d, 64);
            if (lane + d < end) { D.fx += vx; D.fy += vy; D.fz += vz; }
        }
        issue = D.deposit && ((heads >> lane) & 1ull);
    }
    if (issue) deposit_add(A.sums, D);
}

// regen_move_kernel: the compaction's third pass and the film's deposit in one, behind paths_count_kernel and paths_scan_kernel on the same
// records.  A survivor moves as in paths_move_kernel; a retired item is a candidate there and then, from its record (acc in quarter 3,
// pixel in quarter 4), in the deposit's PLAIN form.  Nothing is stored under the id, which may exceed the batch's capacity.  No lane
// leaves before the ballots.
struct RegenMoveArgs {
    const uint4 *items;            // vk_shaded[n]
    const uint32_t *ids;           // [n]
    uint64_t n;
    uint4 *rays;                   // vk_ray[survivors]
    uint4 *states;                 // vk_path_state[survivors]
    uint32_t *ids_out;             // [survivors]
    const uint32_t *wg_offsets;    // [n_wg], paths_scan_kernel's
    unsigned long long *sums;      // the film's [n_pixels * 3]
    unsigned long long *counters;  // the film's deposited, dropped, clamped, skipped
    uint32_t n_pixels;
    float accum_clamp;             // accum_clamp_for(the film's samples_per_pixel)
};
__global__ __launch_bounds__(PATHS_T) void regen_move_kernel(RegenMoveArgs A) {
    __shared__ uint32_t wc[PATHS_T / 64];
    const uint64_t i = (uint64_t)blockIdx.x * PATHS_T + threadIdx.x;
    const Moved R = move_survivor(A, i, wc);
    const bool gone = i < A.n && !R.go;
    uint4 s1 = make_uint4(0u, 0u, 0u, 0u), s2 = s1;
    if (gone) { s1 = A.items[i * 6u + 3u]; s2 = A.items[i * 6u + 4u]; }
    const Deposit D = deposit_lane(gone, R.tail.x, s1, s2, A.n_pixels, A.accum_clamp, A.counters);
    if (D.deposit) deposit_add(A.sums, D);
}

#ifdef VK_DEBUG_LIB
// device math probe (tests: GPU transcendental/draw functions are bit-identical to the host's)
__global__ void math_probe_kernel(int op, const float *a, const float *b, float *out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.0f;
    switch (op) {
        case 0: r = vk::sinf_(a[i]); break;
        case 1: r = vk::cosf_(a[i]); break;
        case 2: r = vk::logf_(a[i]); break;
        case 3: r = vk::asinf_(a[i]); break;
        case 4: r = vk::atan2f_(a[i], b[i]); break;
        case 5: r = vk::pow5f_(a[i]); break;
        case 6: r = a[i] / b[i]; break;
        case 7: r = sqrtf(a[i]); break;
        case 8: { vk::Rng g = vk::rng_for_sample(__float_as_uint(a[i]), (uint32_t)i, 0);
            r = vk::gen_range(g, -1.0f, 1.0f) + vk::gen_f32(g); break; }
        case 9: r = a[i] * b[i] + a[i]; break;   // must stay an unfused mul+add
        case 10: r = div_by_a(a[i], b[i], refined_rcp(b[i]), true); break;      // the sphere test's quotient by a shared reciprocal
        case 11: r = vk::sincosf_(a[i]).s; break;
        case 12: r = vk::sincosf_(a[i]).c; break;
        case 13: r = vk::sincosf_small_(a[i]).s; break;       // (0 <= a < 2^22 only)
        case 14: r = vk::sincosf_small_(a[i]).c; break;
    }
    out[i] = r;
}

#endif

}  // namespace
#endif
