// vk_upsample.hip — the kernels behind vk_upsample_* (include/vecchio_amd.h "guided upsampling"): the prepare pass over the low frame
// and the filter over the high one in its two forms.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the
// handle, the argument checks and AUTO's rule stay in vk_api.hip, which calls the launchers at the end of this file.
//
// The arithmetic is vk_upsample.h's, shared with the host build of tests/emu: upsample_prepare_pixel and upsample_pixel.  The two forms
// differ only in where a tap's three records come from, so they agree bit for bit.
#include <hip/hip_runtime.h>

#include "vk_upsample.h"

namespace {

constexpr int UP_T = 256;                              // 4 waves a workgroup
constexpr int UP_PX = 64, UP_PY = 4;                   // the plain form and prepare: one wave per row of 64 pixels

// fallback_pixels and empty_pixels: one add per wave and count, by the wave's first active lane
__device__ __forceinline__ void up_count(uint32_t *counts, int what) {
    const unsigned long long fb = __ballot(what >= 1), em = __ballot(what == 2);
    if (fb == 0ull) return;
    const unsigned long long active = __ballot(1);
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)active) - 1) {
        atomicAdd(&counts[0], (uint32_t)__popcll(fb));
        if (em) atomicAdd(&counts[1], (uint32_t)__popcll(em));
    }
}

}  // namespace

__global__ __launch_bounds__(UP_T) void upsample_prepare_kernel(UpsamplePrepareArgs A) {
    const uint32_t x = blockIdx.x * UP_PX + (threadIdx.x & 63u), y = blockIdx.y * UP_PY + (threadIdx.x >> 6);
    if (x >= A.w || y >= A.h) return;
    const size_t q = (size_t)y * A.w + x;
    UpRec p0, p1, p2;
    upsample_prepare_pixel(A.color, A.stderr3, A.albedo, A.normal, A.depth, A.albedo_floor, q, p0, p1, p2);
    A.P0[q] = p0; A.P1[q] = p1; A.P2[q] = p2;
}

// PLAIN: one lane per high pixel, its (up to) 16 taps' records straight from global memory: neighbouring lanes share most of them, so
// they come from L1 / L2.
__global__ __launch_bounds__(UP_T) void upsample_plain_kernel(UpsampleArgs A) {
    const int X = (int)(blockIdx.x * UP_PX + (threadIdx.x & 63u)), Y = (int)(blockIdx.y * UP_PY + (threadIdx.x >> 6));
    int what = 0;
    if (X < (int)A.W && Y < (int)A.H)
        what = upsample_pixel(A, X, Y, [&](int tx, int ty, UpRec &q0, UpRec &q1, UpRec &q2) {
            const size_t q = (size_t)ty * A.w + (size_t)tx;
            q0 = A.P0[q]; q1 = A.P1[q]; q2 = A.P2[q];
        });
    up_count(A.counts, what);
}

// TILED: a workgroup owns UP_TX x UP_TY high pixels.  Their taps lie in the low rectangle from (floor(px(X0)) - 1, floor(py(Y0)) - 1),
// at most UP_FW x UP_FH records because the ratio is <= 1 (px is monotone in X: a rounded product of a monotone sum).  The workgroup
// stages the part of it inside the low image in LDS once, 20 736 bytes, and every lane filters from there; a tap outside the staged
// rectangle — there is none by the bound above — would come from global memory, not from beyond the arrays.
__global__ __launch_bounds__(UP_T) void upsample_tiled_kernel(UpsampleArgs A) {
    __shared__ UpRec s0[UP_FW * UP_FH], s1[UP_FW * UP_FH], s2[UP_FW * UP_FH];
    const int tid = (int)threadIdx.x;
    const int X0 = (int)blockIdx.x * UP_TX, Y0 = (int)blockIdx.y * UP_TY;
    const int lx0 = (int)floorf(up_map(X0, A.rx)) - 1, ly0 = (int)floorf(up_map(Y0, A.ry)) - 1;
    for (int i = tid; i < UP_FW * UP_FH; i += UP_T) {
        const int sy = i / UP_FW, sx = i - sy * UP_FW, tx = lx0 + sx, ty = ly0 + sy;
        if (tx < 0 || tx >= (int)A.w || ty < 0 || ty >= (int)A.h) continue;
        const size_t q = (size_t)ty * A.w + (size_t)tx;
        s0[i] = A.P0[q]; s1[i] = A.P1[q]; s2[i] = A.P2[q];
    }
    __syncthreads();
    const int X = X0 + (tid & (UP_TX - 1)), Y = Y0 + tid / UP_TX;
    int what = 0;
    if (X < (int)A.W && Y < (int)A.H)
        what = upsample_pixel(A, X, Y, [&](int tx, int ty, UpRec &q0, UpRec &q1, UpRec &q2) {
            const int sx = tx - lx0, sy = ty - ly0;
            if (sx >= 0 && sx < UP_FW && sy >= 0 && sy < UP_FH) {
                const int i = sy * UP_FW + sx;
                q0 = s0[i]; q1 = s1[i]; q2 = s2[i];
            } else {
                const size_t q = (size_t)ty * A.w + (size_t)tx;
                q0 = A.P0[q]; q1 = A.P1[q]; q2 = A.P2[q];
            }
        });
    up_count(A.counts, what);
}

// ---- the launchers (vk_upsample.h): null stream, current device; sizes >= 2 are the caller's to ensure
void launch_upsample_prepare(const UpsamplePrepareArgs &A) {
    const dim3 grid((A.w + UP_PX - 1) / UP_PX, (A.h + UP_PY - 1) / UP_PY);
    hipLaunchKernelGGL(upsample_prepare_kernel, grid, dim3(UP_T), 0, nullptr, A);
}

void launch_upsample_apply(const UpsampleArgs &A, uint32_t form) {
    if (form == UPSAMPLE_FORM_TILED) {
        const dim3 grid((A.W + UP_TX - 1) / UP_TX, (A.H + UP_TY - 1) / UP_TY);
        hipLaunchKernelGGL(upsample_tiled_kernel, grid, dim3(UP_T), 0, nullptr, A);
    } else {
        const dim3 grid((A.W + UP_PX - 1) / UP_PX, (A.H + UP_PY - 1) / UP_PY);
        hipLaunchKernelGGL(upsample_plain_kernel, grid, dim3(UP_T), 0, nullptr, A);
    }
}
