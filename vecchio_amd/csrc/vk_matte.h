// vk_matte.h — ID mattes (vk_render_mattes, include/vecchio_amd.h): the per-lane pieces, host-and-device (tests/emu/emu_matte.cpp builds
// them with g++; vk_api.hip's vk_matte_merge uses the table's insert and sort on the host), and the kernels of vk_matte.hip as vk_api.hip
// sees them: their argument record and one thin launcher each (the caller checks hipGetLastError).  Nothing here is a float: a sample is
// never dropped, and every result is exact.
#ifndef VK_MATTE_H
#define VK_MATTE_H

#include <stdint.h>

#include "vk_trace.h"       // start_sample_core, begin_segment, the walk, build_record, DProvenance

namespace vkd {

enum : uint32_t { MATTE_OBJECT = 0u, MATTE_MATERIAL = 1u };      // = VK_MATTE_*
constexpr uint32_t MATTE_BACKGROUND = 0xFFFFFFFFu, MATTE_MAX_RANKS = 8u;

// The id of sample `sample` of pixel (x, y): aov_sample's primary ray and walk (start_sample_core, its stream continuing into a
// ConstantMedium's draw; S must be a tree view), then the name of the winner.  MATTE_OBJECT: trace_ray's H.object — the description
// record whose own hit() produced it, through the provenance tables.  MATTE_MATERIAL: the record's material (build_record's R.mat: a
// medium's is its phase function's).  A miss is MATTE_BACKGROUND under either kind.
template <uint32_t F, class Mem>
VK_HD uint32_t matte_sample(Lane &L, const DScene &S, const Mem &M, const DProvenance &P, const RenderConsts &C, uint32_t x, uint32_t y,
    uint32_t sample, uint32_t kind) {
    V3 o, d; float time;
    start_sample_core(L, C, x, y, sample, o, d, time);
    begin_segment<Mem::ISHIFT, fused_box<F, Mem>(), spheres_only<F>()>(L, S, o, d, time);
    while (traversing(L)) traverse_step<F, Mem>(L, S, M);
    if (L.best_prim == 0u) return MATTE_BACKGROUND;
    if (kind == MATTE_MATERIAL) {
        Rec R;
        build_record<F, Mem>(L, S, M, R);
        return R.mat;
    }
    const uint32_t k = VKD_KIND(L.best_prim), idx = VKD_INDEX(L.best_prim);
    if ((F & VKF_MEDIUM) && k == DK_MEDIUM) return VK_MAKE_REF(VK_KIND_MEDIUM, P.medium[idx]);
    if ((F & VKF_BOX) && k == DK_BOX) return VK_MAKE_REF(VK_KIND_RECT, P.box_face[idx * 6u + vk::f32_bits(L.best_aux)]);
    if ((F & VKF_RECT) && k == DK_RECT) return VK_MAKE_REF(VK_KIND_RECT, P.rect[idx]);
    if ((F & VKF_MOVING) && k == DK_MOVING) return VK_MAKE_REF(VK_KIND_MOVING_SPHERE, P.moving[idx]);
    return VK_MAKE_REF(VK_KIND_SPHERE, P.sphere[idx]);
}

// The table of a pixel: eight (id, count) pairs, the first `used` of them taken (count >= 1), the others (0, 0).  Every loop below has
// constant bounds and is unrolled, so on the device each pair is a register pair of its own: an index that is only known at run time
// would put the table in scratch.
struct MatteTable {
    uint32_t id[MATTE_MAX_RANKS], cnt[MATTE_MAX_RANKS];
    uint32_t used, overflow;
};

#if defined(__HIPCC__) || defined(__HIP__)
#define VK_MATTE_UNROLL _Pragma("unroll")
#else
#define VK_MATTE_UNROLL
#endif

VK_HD void matte_clear(MatteTable &T) {
    VK_MATTE_UNROLL
    for (uint32_t r = 0; r < MATTE_MAX_RANKS; r++) { T.id[r] = 0u; T.cnt[r] = 0u; }
    T.used = 0u; T.overflow = 0u;
}

// `c` (>= 1) samples of `id` arrive: its slot takes them; else the first free slot of the `ranks`; else the overflow.  No eviction.
VK_HD void matte_insert(MatteTable &T, uint32_t ranks, uint32_t id, uint32_t c) {
    bool found = false;
    VK_MATTE_UNROLL
    for (uint32_t r = 0; r < MATTE_MAX_RANKS; r++) {
        const bool m = r < T.used && T.id[r] == id;
        T.cnt[r] += m ? c : 0u;
        found = found || m;
    }
    const bool take = !found && T.used < ranks;
    VK_MATTE_UNROLL
    for (uint32_t r = 0; r < MATTE_MAX_RANKS; r++) {
        const bool m = take && r == T.used;
        T.id[r] = m ? id : T.id[r];
        T.cnt[r] = m ? c : T.cnt[r];
    }
    T.used += take ? 1u : 0u;
    T.overflow += (found || take) ? 0u : c;
}

// slot a before slot b: count descending, ties by id ascending (a free slot, (0, 0), after every taken one)
VK_HD void matte_order(uint32_t &ia, uint32_t &ca, uint32_t &ib, uint32_t &cb) {
    const bool swap = cb > ca || (cb == ca && ib < ia);
    const uint32_t i0 = swap ? ib : ia, c0 = swap ? cb : ca, i1 = swap ? ia : ib, c1 = swap ? ca : cb;
    ia = i0; ca = c0; ib = i1; cb = c1;
}
// the 19 comparators of the optimal sorting network on eight inputs, in six layers
VK_HD void matte_sort(MatteTable &T) {
#define VK_MATTE_CE(a, b) matte_order(T.id[a], T.cnt[a], T.id[b], T.cnt[b])
    VK_MATTE_CE(0, 2); VK_MATTE_CE(1, 3); VK_MATTE_CE(4, 6); VK_MATTE_CE(5, 7);
    VK_MATTE_CE(0, 4); VK_MATTE_CE(1, 5); VK_MATTE_CE(2, 6); VK_MATTE_CE(3, 7);
    VK_MATTE_CE(0, 1); VK_MATTE_CE(2, 3); VK_MATTE_CE(4, 5); VK_MATTE_CE(6, 7);
    VK_MATTE_CE(2, 4); VK_MATTE_CE(3, 5);
    VK_MATTE_CE(1, 4); VK_MATTE_CE(3, 6);
    VK_MATTE_CE(1, 2); VK_MATTE_CE(3, 4); VK_MATTE_CE(5, 6);
#undef VK_MATTE_CE
}

}  // namespace vkd

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// matte_kernel<F> and matte_samples_kernel<F>: aov_kernel's launch shape (one 8x8 tile per wave, 256 lanes a workgroup) over the call's
// tile partition
struct MatteArgs {
    vkd::DScene S;           // a tree view (vk_api.hip aov_view)
    vkd::DProvenance P;
    vkd::RenderConsts C;     // C.spp = the window's length; the background and the integrator are not read
    uint32_t *ids, *counts;  // [width * height * ranks], 16-byte aligned (matte_kernel); ids alone [width * height * spp] (the samples)
    uint32_t *overflow;      // [width * height], may be null
    uint32_t kind, ranks;
    uint32_t first_sample, tiles_x, tile_rank, tile_world, n_local;
};
constexpr int MATTE_BLOCK = 256;     // 4 waves = 4 tiles per workgroup

// null stream, current device, A.n_local > 0.  features: the scene's (0: the sphere-only instance, else the everything-variant)
void launch_matte(uint32_t features, const MatteArgs &A);
void launch_matte_samples(uint32_t features, const MatteArgs &A);      // the per-sample kernel of vk_debug_matte_samples
#endif

#endif
