// vk_matte.hip — the kernels behind vk_render_mattes and vk_debug_matte_samples (include/vecchio_amd.h, "ID mattes"): which object, or
// which material, the primary rays of a pixel's samples show, as a small ranked table per pixel.  A translation unit of its own
// (vk_kernels.h belongs to vk_api.hip): the C ABI, the checks and the staging stay in vk_api.hip, which calls the launchers at the end
// of this file.
//
// Launch shape: aov_kernel's.  One 8x8 tile per wave (coherent primary rays), 256 lanes a workgroup, the samples of a pixel in increasing
// order inside its lane, the walk vk_trace.h's per-lane one on GlobalMem.  The table lives in registers across the walk (vk_matte.h: eight
// (id, count) pairs, compare-and-select only); no LDS, no atomics.  Every value is an integer and the order of a pixel's samples is
// fixed: the result does not depend on the launch shape.
#include <hip/hip_runtime.h>

#include "vk_emit.h"        // TILE
#include "vk_matte.h"

namespace {

// the lane's pixel of the call's tile partition; false: no such tile, or the pixel lies outside the frame
__device__ __forceinline__ bool matte_pixel(const MatteArgs &A, uint32_t &x, uint32_t &y) {
    const uint32_t lane = threadIdx.x & 63u, local = blockIdx.x * (MATTE_BLOCK / 64) + (threadIdx.x >> 6);
    if (local >= A.n_local) return false;
    const uint32_t tile = A.tile_rank + local * A.tile_world;
    x = (tile % A.tiles_x) * TILE + (lane & 7u); y = (tile / A.tiles_x) * TILE + (lane >> 3);
    return x < A.C.width && y < A.C.height;
}

// One pixel's table over samples [first_sample, first_sample + C.spp).  The stores are as wide as `ranks` allows: ranks 4 and 8 write
// 16 bytes at a time (the arrays are 16-byte aligned and a pixel's slots start at pix * ranks words), ranks 2 and 6 eight.
template <uint32_t F>
__global__ __launch_bounds__(MATTE_BLOCK) void matte_kernel(MatteArgs A) {
    uint32_t x, y;
    if (!matte_pixel(A, x, y)) return;
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    MatteTable T;
    matte_clear(T);
#pragma unroll 1
    for (uint32_t k = 0; k < A.C.spp; k++) {
        Lane L;
        const uint32_t id = matte_sample<F, GlobalMem>(L, A.S, M, A.P, A.C, x, y, A.first_sample + k, A.kind);
        matte_insert(T, A.ranks, id, 1u);
    }
    matte_sort(T);
    const size_t pix = (size_t)y * A.C.width + x;
    uint32_t *ids = A.ids + pix * A.ranks, *cnt = A.counts + pix * A.ranks;
    if ((A.ranks & 3u) == 0u) {
        reinterpret_cast<uint4 *>(ids)[0] = make_uint4(T.id[0], T.id[1], T.id[2], T.id[3]);
        reinterpret_cast<uint4 *>(cnt)[0] = make_uint4(T.cnt[0], T.cnt[1], T.cnt[2], T.cnt[3]);
        if (A.ranks == 8u) {
            reinterpret_cast<uint4 *>(ids)[1] = make_uint4(T.id[4], T.id[5], T.id[6], T.id[7]);
            reinterpret_cast<uint4 *>(cnt)[1] = make_uint4(T.cnt[4], T.cnt[5], T.cnt[6], T.cnt[7]);
        }
    } else if ((A.ranks & 1u) == 0u) {
        reinterpret_cast<uint2 *>(ids)[0] = make_uint2(T.id[0], T.id[1]);
        reinterpret_cast<uint2 *>(cnt)[0] = make_uint2(T.cnt[0], T.cnt[1]);
        if (A.ranks == 6u) {
            reinterpret_cast<uint2 *>(ids)[1] = make_uint2(T.id[2], T.id[3]);
            reinterpret_cast<uint2 *>(cnt)[1] = make_uint2(T.cnt[2], T.cnt[3]);
            reinterpret_cast<uint2 *>(ids)[2] = make_uint2(T.id[4], T.id[5]);
            reinterpret_cast<uint2 *>(cnt)[2] = make_uint2(T.cnt[4], T.cnt[5]);
        }
    } else {
#pragma unroll
        for (uint32_t r = 0; r < MATTE_MAX_RANKS - 1u; r++)
            if (r < A.ranks) { ids[r] = T.id[r]; cnt[r] = T.cnt[r]; }
    }
    if (A.overflow) A.overflow[pix] = T.overflow;
}

// vk_debug_matte_samples: the same lanes, each sample's id stored instead of counted — ids[(pix * spp) + k]
template <uint32_t F>
__global__ __launch_bounds__(MATTE_BLOCK) void matte_samples_kernel(MatteArgs A) {
    uint32_t x, y;
    if (!matte_pixel(A, x, y)) return;
    const GlobalMem M{A.S.items, A.S.spheres, A.S.sphere_mat, A.S.boxes};
    uint32_t *out = A.ids + ((size_t)y * A.C.width + x) * A.C.spp;
#pragma unroll 1
    for (uint32_t k = 0; k < A.C.spp; k++) {
        Lane L;
        out[k] = matte_sample<F, GlobalMem>(L, A.S, M, A.P, A.C, x, y, A.first_sample + k, A.kind);
    }
}

dim3 matte_grid(const MatteArgs &A) { return dim3((A.n_local + MATTE_BLOCK / 64 - 1) / (MATTE_BLOCK / 64)); }

}  // namespace

// ---- the launchers (vk_matte.h): the two instances the first-hit kernels have
void launch_matte(uint32_t features, const MatteArgs &A) {
    if (features == 0u) hipLaunchKernelGGL(matte_kernel<0u>, matte_grid(A), dim3(MATTE_BLOCK), 0, nullptr, A);
    else hipLaunchKernelGGL(matte_kernel<(uint32_t)VKF_ALL_SCENE>, matte_grid(A), dim3(MATTE_BLOCK), 0, nullptr, A);
}
void launch_matte_samples(uint32_t features, const MatteArgs &A) {
    if (features == 0u) hipLaunchKernelGGL(matte_samples_kernel<0u>, matte_grid(A), dim3(MATTE_BLOCK), 0, nullptr, A);
    else hipLaunchKernelGGL(matte_samples_kernel<(uint32_t)VKF_ALL_SCENE>, matte_grid(A), dim3(MATTE_BLOCK), 0, nullptr, A);
}
