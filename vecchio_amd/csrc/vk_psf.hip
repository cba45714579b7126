// vk_psf.hip — the kernels behind vk_psf_* (include/vecchio_amd.h "point-spread function"): a 2-D radix-2 FFT over planes of complex
// f32, the pointwise product with the loaded kernel's transform and the composite.  A translation unit of its own (vk_kernels.h belongs
// to vk_api.hip): the C ABI, the handle, the argument checks and the launch plan stay in vk_api.hip, which calls the launchers at the
// end of this file.
//
// The arithmetic is vk_psf.h's, shared with the host build of tests/emu: psf_bright, psf_mul, psf_butterfly, psf_composite.  Both forms
// run the same butterflies on the same values; only which lane runs which, and where the line lives meanwhile, differ, so the forms
// agree bit for bit (the sign of a zero aside: the LDS form never computes the rows that are all zero).
#include <hip/hip_runtime.h>

#include "vk_psf.h"

namespace {

constexpr int PSF_T = 256;                             // 4 waves a workgroup

}  // namespace

// psf_pad_kernel: one lane per value of a plane, all three planes
__global__ __launch_bounds__(PSF_T) void psf_pad_kernel(PsfPadArgs A) {
    const uint32_t x = blockIdx.x * (uint32_t)PSF_T + threadIdx.x, y = blockIdx.y;
    if (x >= A.Px || y >= A.Py) return;
    float B[3] = {0.0f, 0.0f, 0.0f};
    if (x < A.W && y < A.H) {
        const size_t p = ((size_t)y * A.W + x) * 3u;
        const float I[3] = {A.in[p], A.in[p + 1], A.in[p + 2]};
        psf_bright(I, A.threshold, B);
    }
    const size_t n = (size_t)A.Px * A.Py, q = (size_t)y * A.Px + x;
#pragma unroll
    for (int c = 0; c < 3; c++) A.F[(size_t)c * n + q] = PsfC{B[c], 0.0f};
}

// psf_place_kernel: one lane per value of a plane, all three planes
__global__ __launch_bounds__(PSF_T) void psf_place_kernel(PsfPlaceArgs A) {
    const uint32_t x = blockIdx.x * (uint32_t)PSF_T + threadIdx.x, y = blockIdx.y;
    if (x >= A.Px || y >= A.Py) return;
    const size_t n = (size_t)A.Px * A.Py, q = (size_t)y * A.Px + x;
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) A.G[(size_t)c * n + q] = PsfC{psf_placed(A.kernel, A.K, c, A.Px, A.Py, x, y), 0.0f};
}

// psf_bitrev_kernel: one lane per value; the lane of the smaller index of a pair swaps it.  blockIdx.z = the plane.
__global__ __launch_bounds__(PSF_T) void psf_bitrev_kernel(PsfStageArgs A) {
    const uint32_t x = blockIdx.x * (uint32_t)PSF_T + threadIdx.x, y = blockIdx.y;
    if (x >= A.Px || y >= A.Py) return;
    PsfC *a = A.a + (size_t)blockIdx.z * A.Px * A.Py;
    const uint32_t N = A.axis ? A.Py : A.Px, m = 31u - (uint32_t)__clz((int)N), i = A.axis ? y : x;
    const uint32_t j = m ? __brev(i) >> (32u - m) : 0u;
    if (i >= j) return;
    const size_t p = (size_t)y * A.Px + x, q = A.axis ? (size_t)j * A.Px + x : (size_t)y * A.Px + j;
    const PsfC t = a[p];
    a[p] = a[q];
    a[q] = t;
}

// psf_stage_kernel: one lane per butterfly of the stage: along x, lane (i, y) of Px/2 x Py; along y, lane (x, i) of Px x Py/2
__global__ __launch_bounds__(PSF_T) void psf_stage_kernel(PsfStageArgs A) {
    const uint32_t gx = blockIdx.x * (uint32_t)PSF_T + threadIdx.x, gy = blockIdx.y;
    const uint32_t nx = A.axis ? A.Px : A.Px / 2u, ny = A.axis ? A.Py / 2u : A.Py;
    if (gx >= nx || gy >= ny) return;
    PsfC *a = A.a + (size_t)blockIdx.z * A.Px * A.Py;
    const uint32_t N = A.axis ? A.Py : A.Px, m = 31u - (uint32_t)__clz((int)N);
    uint32_t p, half, wk;
    psf_butterfly_at(A.axis ? gy : gx, A.s, m, p, half, wk);
    const size_t iu = A.axis ? (size_t)p * A.Px + gx : (size_t)gy * A.Px + p;
    const size_t iv = A.axis ? (size_t)(p + half) * A.Px + gx : iu + half;
    PsfC u = a[iu], v = a[iv];
    psf_butterfly(u, v, A.T[wk], A.inverse != 0u);
    a[iu] = u;
    a[iv] = v;
}

__global__ __launch_bounds__(PSF_T) void psf_product_kernel(PsfProductArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * (uint64_t)PSF_T + threadIdx.x;
    if (i >= A.n) return;
    A.F[i] = psf_mul(A.F[i], A.G[i]);
}

__global__ __launch_bounds__(PSF_T) void psf_scale_kernel(PsfScaleArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * (uint64_t)PSF_T + threadIdx.x;
    if (i >= A.n) return;
    PsfC v = A.a[i];
    v.re *= A.scale; v.im *= A.scale;
    A.a[i] = v;
}

// psf_composite_kernel: one lane per pixel of the frame; reads its own pixel of the input only, so out may be the input
__global__ __launch_bounds__(PSF_T) void psf_composite_kernel(PsfCompositeArgs A) {
    const uint32_t x = blockIdx.x * (uint32_t)PSF_T + threadIdx.x, y = blockIdx.y;
    if (x >= A.W || y >= A.H) return;
    const size_t p = ((size_t)y * A.W + x) * 3u, n = (size_t)A.Px * A.Py, q = (size_t)y * A.Px + x;
    const float I[3] = {A.in[p], A.in[p + 1], A.in[p + 2]};
    float B[3];
    psf_bright(I, A.threshold, B);
#pragma unroll
    for (int c = 0; c < 3; c++) A.out[p + c] = psf_composite(I[c], B[c], A.F[(size_t)c * n + q].re, A.scale, A.strength);
}

// psf_line_kernel<COL>.  A workgroup takes `lines` whole lines of one plane (blockIdx.y): rows (COL false: the line runs along x, LDS
// slot line * N + pos) or adjacent columns (COL true: the line runs along y, LDS slot pos * lines + line).  Either way consecutive
// lanes touch consecutive 8-byte slots in every stage from half * lines >= 32 on (ds_read_b64, conflict-free: a half-wave covers one
// 256-byte bank row) and every other slot pair below that (2-way); no stage strides by a power of two across lanes, so the lines need no
// padding.  Global memory is read and written along x: a row at a time, or `lines` adjacent values of each row of the column tile.
//
// Load puts value pos at slot rev(pos); then stage s = 1 .. m, a barrier between stages; store in natural order.
template <bool COL>
__global__ __launch_bounds__(PSF_T) void psf_line_kernel(PsfLineArgs A) {
    constexpr uint32_t CAP = COL ? PSF_COL_CAP : PSF_ROW_CAP;
    __shared__ PsfC sA[CAP];
    const uint32_t tid = threadIdx.x;
    const uint32_t N = COL ? A.Py : A.Px, m = 31u - (uint32_t)__clz((int)N);
    const uint32_t L = A.lines, lL = 31u - (uint32_t)__clz((int)L);
    const uint32_t line0 = blockIdx.x * L, ch = blockIdx.y;
    const size_t plane = (size_t)ch * A.Px * A.Py;
    const uint32_t total = L << m;                         // <= CAP: the launcher's caller ensures it
    // where element e of the tile is: (line, pos), its value's place in the plane and its LDS slot
    auto split = [&](uint32_t e, uint32_t &line, uint32_t &pos) {
        if (COL) { line = e & (L - 1u); pos = e >> lL; } else { line = e >> m; pos = e & (N - 1u); }
    };
    auto slot = [&](uint32_t line, uint32_t pos) { return COL ? pos * L + line : (line << m) + pos; };
    for (uint32_t e = tid; e < total; e += (uint32_t)PSF_T) {
        uint32_t line, pos;
        split(e, line, pos);
        const uint32_t gl = line0 + line;
        PsfC v = {0.0f, 0.0f};
        if (gl < A.count) {
            const uint32_t x = COL ? gl : pos, y = COL ? pos : gl;
            const size_t q = plane + (size_t)y * A.Px + x;
            if (A.load == PSF_LOAD_PLANE) {
                v = A.a[q];
            } else if (A.load == PSF_LOAD_PRODUCT) {
                v = psf_mul(A.a[q], A.G[q]);
            } else if (A.load == PSF_LOAD_ROWS) {
                if (y < A.valid) v = A.a[q];
            } else if (x < A.W && y < A.H) {               // PSF_LOAD_FRAME
                const size_t p = ((size_t)y * A.W + x) * 3u;
                const float I[3] = {A.in[p], A.in[p + 1], A.in[p + 2]};
                float B[3];
                psf_bright(I, A.threshold, B);
                v.re = B[ch];
            }
        }
        const uint32_t rp = m ? __brev(pos) >> (32u - m) : 0u;
        sA[slot(line, rp)] = v;
    }
    __syncthreads();
    const bool inverse = A.inverse != 0u;
    for (uint32_t s = 1u; s <= m; s++) {
        for (uint32_t e = tid; e < total / 2u; e += (uint32_t)PSF_T) {
            uint32_t line, i;
            if (COL) { line = e & (L - 1u); i = e >> lL; } else { line = e >> (m - 1u); i = e & (N / 2u - 1u); }
            uint32_t p, half, wk;
            psf_butterfly_at(i, s, m, p, half, wk);
            const uint32_t iu = slot(line, p), iv = slot(line, p + half);
            PsfC u = sA[iu], v = sA[iv];
            psf_butterfly(u, v, A.T[wk], inverse);
            sA[iu] = u;
            sA[iv] = v;
        }
        __syncthreads();
    }
    for (uint32_t e = tid; e < total; e += (uint32_t)PSF_T) {
        uint32_t line, pos;
        split(e, line, pos);
        const uint32_t gl = line0 + line;
        if (gl >= A.count) continue;
        const uint32_t x = COL ? gl : pos, y = COL ? pos : gl;
        PsfC v = sA[slot(line, pos)];
        if (A.store == PSF_STORE_FRAME) {
            if (x >= A.W || y >= A.H) continue;
            const size_t p = ((size_t)y * A.W + x) * 3u;
            const float I[3] = {A.in[p], A.in[p + 1], A.in[p + 2]};
            float B[3];
            psf_bright(I, A.threshold, B);
            A.out[p + ch] = psf_composite(I[ch], B[ch], v.re, A.scale, A.strength);
            continue;
        }
        if (A.store == PSF_STORE_SCALED) { v.re *= A.scale; v.im *= A.scale; }
        A.a[plane + (size_t)y * A.Px + x] = v;
    }
}

// ---- the launchers (vk_psf.h): null stream, current device; sizes > 0, powers of two and within the caps are the caller's to ensure
namespace {

dim3 plane_grid(uint32_t nx, uint32_t ny, uint32_t nz) { return dim3((nx + PSF_T - 1) / PSF_T, ny, nz); }

}  // namespace

void launch_psf_pad(const PsfPadArgs &A) {
    hipLaunchKernelGGL(psf_pad_kernel, plane_grid(A.Px, A.Py, 1u), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_place(const PsfPlaceArgs &A) {
    hipLaunchKernelGGL(psf_place_kernel, plane_grid(A.Px, A.Py, 1u), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_bitrev(const PsfStageArgs &A) {
    hipLaunchKernelGGL(psf_bitrev_kernel, plane_grid(A.Px, A.Py, A.planes), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_stage(const PsfStageArgs &A) {
    const uint32_t nx = A.axis ? A.Px : A.Px / 2u, ny = A.axis ? A.Py / 2u : A.Py;
    hipLaunchKernelGGL(psf_stage_kernel, plane_grid(nx, ny, A.planes), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_product(const PsfProductArgs &A) {
    hipLaunchKernelGGL(psf_product_kernel, dim3((unsigned)((A.n + PSF_T - 1) / PSF_T)), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_scale(const PsfScaleArgs &A) {
    hipLaunchKernelGGL(psf_scale_kernel, dim3((unsigned)((A.n + PSF_T - 1) / PSF_T)), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_composite(const PsfCompositeArgs &A) {
    hipLaunchKernelGGL(psf_composite_kernel, plane_grid(A.W, A.H, 1u), dim3(PSF_T), 0, nullptr, A);
}

void launch_psf_line(const PsfLineArgs &A, bool col) {
    const dim3 grid((A.count + A.lines - 1u) / A.lines, A.planes);
    if (col) hipLaunchKernelGGL(psf_line_kernel<true>, grid, dim3(PSF_T), 0, nullptr, A);
    else hipLaunchKernelGGL(psf_line_kernel<false>, grid, dim3(PSF_T), 0, nullptr, A);
}
