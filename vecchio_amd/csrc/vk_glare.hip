// vk_glare.hip — the kernels behind vk_glare_* (include/vecchio_amd.h "glare"): the down passes of the bright part's pyramid, the up
// passes of the weighted sums and the composite.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the
// handle, the argument checks and the launch plan stay in vk_api.hip, which calls the launchers at the end of this file.
//
// The arithmetic is vk_glare.h's, shared with the host build of tests/emu: glare_bright, glare_down4, glare_up2.  Every kernel applies
// them to the same values in the same order — x first, then y —, so the forms agree bit for bit.
#include <hip/hip_runtime.h>

#include "vk_glare.h"

namespace {

constexpr int GL_T = 256;                              // 4 waves a workgroup
constexpr int GL_PX = 64, GL_PY = 4;                   // the per-pixel kernels: one wave per row of 64 pixels
constexpr int GL_TX = 32, GL_TY = 8;                   // the LDS down kernel's output tile; its source is (2 TX + 2) x (2 TY + 2)
constexpr int GL_SW = 2 * GL_TX + 2, GL_SH = 2 * GL_TY + 2;
constexpr int GL_2X = 16, GL_2Y = 8;                   // the two-level kernel's tile of level 2
constexpr int GL_1W = 2 * GL_2X + 2, GL_1H = 2 * GL_2Y + 2;        // its tile of level 1 with the halo: 34 x 18
constexpr int GL_0W = 2 * GL_1W + 2, GL_0H = 2 * GL_1H + 2;        // its tile of the frame with the halo: 70 x 38
constexpr int GL_TAIL_T = 1024;                        // the tail: 16 waves, one workgroup per colour component

}  // namespace

// glare_down_kernel<BRIGHT, LDS>.
//
// Plain: one lane per pixel of the destination, sixteen source pixels each straight from global memory (glare_down_pixel).
//
// LDS: a workgroup owns GL_TX x GL_TY pixels of the destination.  It stages their source tile and the one-pixel halo in LDS, a slot per
// raw coordinate holding the pixel at the clamped one (component planes: a lane's reads are dwords), runs the x pass over every staged
// row into LDS and the y pass from there: a source pixel is read from memory (and its bright part taken) once, not up to four times.
template <bool BRIGHT, bool LDS>
__global__ __launch_bounds__(GL_T) void glare_down_kernel(GlareDownArgs A) {
    const int sw = (int)A.sw, sh = (int)A.sh, dw = glare_half(sw), dh = glare_half(sh);
    if constexpr (!LDS) {
        const int X = (int)(blockIdx.x * GL_PX + (threadIdx.x & 63u)), Y = (int)(blockIdx.y * GL_PY + (threadIdx.x >> 6));
        if (X >= dw || Y >= dh) return;
        float out[3];
        glare_down_pixel<BRIGHT>(A.src, sw, sh, A.threshold, X, Y, out);
        const size_t p = ((size_t)Y * (size_t)dw + (size_t)X) * 3u;
        A.dst[p] = out[0]; A.dst[p + 1] = out[1]; A.dst[p + 2] = out[2];
    } else {
        __shared__ float sS[3][GL_SW * GL_SH], sX[3][GL_TX * GL_SH];
        const int tid = (int)threadIdx.x;
        const int X0 = (int)blockIdx.x * GL_TX, Y0 = (int)blockIdx.y * GL_TY, gx0 = 2 * X0 - 1, gy0 = 2 * Y0 - 1;
        for (int i = tid; i < GL_SW * GL_SH; i += GL_T) {
            const int sy = i / GL_SW, sx = i - sy * GL_SW;
            float v[3];
            glare_source<BRIGHT>(A.src, sw, glare_clamp(gx0 + sx, sw), glare_clamp(gy0 + sy, sh), A.threshold, v);
            sS[0][i] = v[0]; sS[1][i] = v[1]; sS[2][i] = v[2];
        }
        __syncthreads();
        for (int i = tid; i < 3 * GL_TX * GL_SH; i += GL_T) {
            const int c = i / (GL_TX * GL_SH), r = i - c * (GL_TX * GL_SH), ry = r / GL_TX, rx = r - ry * GL_TX;
            const float *s = &sS[c][ry * GL_SW + 2 * rx];
            sX[c][r] = glare_down4(s[0], s[1], s[2], s[3]);
        }
        __syncthreads();
        const int tx = tid & (GL_TX - 1), ty = tid / GL_TX, X = X0 + tx, Y = Y0 + ty;
        if (X >= dw || Y >= dh) return;
        const size_t p = ((size_t)Y * (size_t)dw + (size_t)X) * 3u;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *s = &sX[c][(2 * ty) * GL_TX + tx];
            A.dst[p + c] = glare_down4(s[0], s[GL_TX], s[2 * GL_TX], s[3 * GL_TX]);
        }
    }
}

// glare_down2_kernel: B_1 and B_2 from the frame.  A workgroup owns GL_2X x GL_2Y pixels of level 2, hence 32 x 16 of level 1, which it
// also writes.  Staged: the frame's 70 x 38 bright pixels under the tile (a slot per raw coordinate, the pixel at the clamped one); the
// x pass of those rows for the tile's 34 columns of level 1; level 1's 34 x 18 tile (a slot per raw coordinate again: slot i holds level
// 1 at clamp(i), made from the staged slots around 2 clamp(i), which the tile holds because it meets the image); level 2's x pass.
__global__ __launch_bounds__(GL_T) void glare_down2_kernel(GlareDown2Args A) {
    __shared__ float sS[3][GL_0W * GL_0H], sX[3][GL_1W * GL_0H], s1[3][GL_1W * GL_1H], sX2[3][GL_2X * GL_1H];
    const int w0 = (int)A.sw, h0 = (int)A.sh, w1 = glare_half(w0), h1 = glare_half(h0), w2 = glare_half(w1), h2 = glare_half(h1);
    const int tid = (int)threadIdx.x;
    const int X0 = (int)blockIdx.x * GL_2X, Y0 = (int)blockIdx.y * GL_2Y;
    const int i0 = 2 * X0 - 1, j0 = 2 * Y0 - 1;              // level 1's raw coordinate of slot 0
    const int gx0 = 2 * i0 - 1, gy0 = 2 * j0 - 1;            // the frame's
    for (int i = tid; i < GL_0W * GL_0H; i += GL_T) {
        const int sy = i / GL_0W, sx = i - sy * GL_0W;
        float v[3];
        glare_source<true>(A.src, w0, glare_clamp(gx0 + sx, w0), glare_clamp(gy0 + sy, h0), A.threshold, v);
        sS[0][i] = v[0]; sS[1][i] = v[1]; sS[2][i] = v[2];
    }
    __syncthreads();
    for (int i = tid; i < 3 * GL_1W * GL_0H; i += GL_T) {
        const int c = i / (GL_1W * GL_0H), r = i - c * (GL_1W * GL_0H), sy = r / GL_1W, ix = r - sy * GL_1W;
        const int ci = glare_clamp(i0 + ix, w1) - i0;        // in 0 .. GL_1W - 1
        const float *s = &sS[c][sy * GL_0W + 2 * ci];
        sX[c][r] = glare_down4(s[0], s[1], s[2], s[3]);
    }
    __syncthreads();
    for (int i = tid; i < 3 * GL_1W * GL_1H; i += GL_T) {
        const int c = i / (GL_1W * GL_1H), r = i - c * (GL_1W * GL_1H), jy = r / GL_1W, ix = r - jy * GL_1W;
        const int cj = glare_clamp(j0 + jy, h1) - j0;        // in 0 .. GL_1H - 1
        const float *s = &sX[c][(2 * cj) * GL_1W + ix];
        const float v = glare_down4(s[0], s[GL_1W], s[2 * GL_1W], s[3 * GL_1W]);
        s1[c][r] = v;
        const int x1 = i0 + ix, y1 = j0 + jy;
        if (ix >= 1 && ix <= 2 * GL_2X && jy >= 1 && jy <= 2 * GL_2Y && x1 < w1 && y1 < h1)
            A.b1[((size_t)y1 * (size_t)w1 + (size_t)x1) * 3u + (size_t)c] = v;
    }
    __syncthreads();
    for (int i = tid; i < 3 * GL_2X * GL_1H; i += GL_T) {
        const int c = i / (GL_2X * GL_1H), r = i - c * (GL_2X * GL_1H), jy = r / GL_2X, rx = r - jy * GL_2X;
        const float *s = &s1[c][jy * GL_1W + 2 * rx];
        sX2[c][r] = glare_down4(s[0], s[1], s[2], s[3]);
    }
    __syncthreads();
    for (int i = tid; i < 3 * GL_2X * GL_2Y; i += GL_T) {
        const int c = i / (GL_2X * GL_2Y), r = i - c * (GL_2X * GL_2Y), ty = r / GL_2X, tx = r - ty * GL_2X;
        const int X = X0 + tx, Y = Y0 + ty;
        if (X >= w2 || Y >= h2) continue;
        const float *s = &sX2[c][(2 * ty) * GL_2X + tx];
        A.b2[((size_t)Y * (size_t)w2 + (size_t)X) * 3u + (size_t)c] = glare_down4(s[0], s[GL_2X], s[2 * GL_2X], s[3 * GL_2X]);
    }
}

// glare_up_kernel: one lane per pixel of level l: A_l = c_l * B_l + Up(scale * src)
__global__ __launch_bounds__(GL_T) void glare_up_kernel(GlareUpArgs A) {
    const int x = (int)(blockIdx.x * GL_PX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * GL_PY + (threadIdx.x >> 6));
    const int w = (int)A.w, h = (int)A.h;
    if (x >= w || y >= h) return;
    float up[3];
    glare_up_pixel(A.src, glare_half(w), glare_half(h), A.scale, x, y, up);
    const size_t p = ((size_t)y * (size_t)w + (size_t)x) * 3u;
#pragma unroll
    for (int c = 0; c < 3; c++) A.dst[p + c] = A.c * A.b[p + c] + up[c];
}

// glare_composite_kernel: one lane per pixel of the frame; reads its own pixel of the input only, so out may be the input
__global__ __launch_bounds__(GL_T) void glare_composite_kernel(GlareCompositeArgs A) {
    const int x = (int)(blockIdx.x * GL_PX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * GL_PY + (threadIdx.x >> 6));
    const int w = (int)A.w, h = (int)A.h;
    if (x >= w || y >= h) return;
    const size_t p = ((size_t)y * (size_t)w + (size_t)x) * 3u;
    const float I[3] = {A.in[p], A.in[p + 1], A.in[p + 2]};
    float up[3] = {0.0f, 0.0f, 0.0f}, out[3];
    if (A.src) glare_up_pixel(A.src, glare_half(w), glare_half(h), A.scale, x, y, up);
    glare_composite_pixel(I, A.threshold, A.c0, A.strength, A.src != nullptr, up, out);
    A.out[p] = out[0]; A.out[p + 1] = out[1]; A.out[p + 2] = out[2];
}

namespace {

// one output of the down filter at (X, Y) over a(x, y), x first; one of the up filter at (x, y)
template <typename F>
__device__ __forceinline__ float tail_down(F a, int sw, int sh, int X, int Y) {
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int y = glare_clamp(2 * Y - 1 + k, sh);
        r[k] = glare_down4(a(glare_clamp(2 * X - 1, sw), y), a(glare_clamp(2 * X, sw), y), a(glare_clamp(2 * X + 1, sw), y),
                           a(glare_clamp(2 * X + 2, sw), y));
    }
    return glare_down4(r[0], r[1], r[2], r[3]);
}

template <typename F>
__device__ __forceinline__ float tail_up(F a, int sw, int sh, int x, int y) {
    const int jx = x >> 1, nx = glare_up_nb(x, sw), jy = y >> 1, ny = glare_up_nb(y, sh);
    return glare_up2(glare_up2(a(jx, jy), a(nx, jy)), glare_up2(a(jx, ny), a(nx, ny)));
}

// level l's size from level t's, and where B_l (l > t) begins in the tail's B store
__device__ __forceinline__ void tail_level(int wt, int ht, uint32_t t, uint32_t l, int &w, int &h, int &off) {
    w = wt; h = ht; off = 0;
    for (uint32_t k = t; k < l; k++) {
        if (k > t) off += w * h;
        w = glare_half(w); h = glare_half(h);
    }
}

}  // namespace

// glare_tail_kernel: levels t .. L - 1 by one workgroup per colour component (blockIdx.x), t + 2 <= L.  B_{t+1} .. B_{L-1} are made in
// LDS, side by side in sB, each from the level below (B_t from global memory); then A_{L-2} .. A_{t+1} in sA and sA2 by turns, A_{t+1}
// in sA; A_t goes to global memory.  A_{L-1} = c_{L-1} * B_{L-1} is taken as it is read.  The launcher's caller ensures the sizes fit
// (glare_tail_level).
__global__ __launch_bounds__(GL_TAIL_T) void glare_tail_kernel(GlareTailArgs A) {
    __shared__ float sB[GLARE_TAIL_B], sA[GLARE_TAIL_A], sA2[GLARE_TAIL_A2];
    const int tid = (int)threadIdx.x, ch = (int)blockIdx.x;
    const int wt = (int)A.w, ht = (int)A.h;
    const uint32_t t = A.t, L = A.levels;
    const float *bt = A.bt + ch;
    // down: B_{l+1} from B_l, l = t .. L - 2
    for (uint32_t l = t; l + 1u < L; l++) {
        int sw, sh, soff, dw, dh, doff;
        tail_level(wt, ht, t, l, sw, sh, soff);
        tail_level(wt, ht, t, l + 1u, dw, dh, doff);
        float *dst = sB + doff;
        if (l == t) {
            for (int i = tid; i < dw * dh; i += GL_TAIL_T) {
                const int Y = i / dw, X = i - Y * dw;
                dst[i] = tail_down([&](int x, int y) { return bt[((size_t)y * (size_t)sw + (size_t)x) * 3u]; }, sw, sh, X, Y);
            }
        } else {
            const float *src = sB + soff;
            for (int i = tid; i < dw * dh; i += GL_TAIL_T) {
                const int Y = i / dw, X = i - Y * dw;
                dst[i] = tail_down([&](int x, int y) { return src[y * sw + x]; }, sw, sh, X, Y);
            }
        }
        __syncthreads();
    }
    // up: A_l = c_l * B_l + Up(A_{l+1}), l = L - 2 .. t
    for (uint32_t l = L - 2u;; l--) {
        int w, h, off, sw, sh, soff;
        tail_level(wt, ht, t, l, w, h, off);
        tail_level(wt, ht, t, l + 1u, sw, sh, soff);
        const bool top = l + 2u == L;
        const float *src = top ? sB + soff : (((l + 1u - (t + 1u)) & 1u) ? sA2 : sA);
        const float scale = top ? A.c[L - 1u] : 1.0f, cl = A.c[l];
        auto a = [&](int x, int y) { return scale * src[y * sw + x]; };
        if (l == t) {
            for (int i = tid; i < w * h; i += GL_TAIL_T) {
                const int y = i / w, x = i - y * w;
                const size_t p = (size_t)i * 3u + (size_t)ch;
                A.at[p] = cl * A.bt[p] + tail_up(a, sw, sh, x, y);
            }
            break;
        }
        float *dst = ((l - (t + 1u)) & 1u) ? sA2 : sA;
        const float *b = sB + off;
        for (int i = tid; i < w * h; i += GL_TAIL_T) {
            const int y = i / w, x = i - y * w;
            dst[i] = cl * b[i] + tail_up(a, sw, sh, x, y);
        }
        __syncthreads();
    }
}

// ---- the launchers (vk_glare.h): null stream, current device; sizes > 0 and the plan's preconditions are the caller's to ensure
void launch_glare_down(const GlareDownArgs &A, bool bright, bool lds) {
    const uint32_t dw = (A.sw + 1u) / 2u, dh = (A.sh + 1u) / 2u;
    if (lds) {
        const dim3 grid((dw + GL_TX - 1) / GL_TX, (dh + GL_TY - 1) / GL_TY);
        if (bright) hipLaunchKernelGGL((glare_down_kernel<true, true>), grid, dim3(GL_T), 0, nullptr, A);
        else hipLaunchKernelGGL((glare_down_kernel<false, true>), grid, dim3(GL_T), 0, nullptr, A);
    } else {
        const dim3 grid((dw + GL_PX - 1) / GL_PX, (dh + GL_PY - 1) / GL_PY);
        if (bright) hipLaunchKernelGGL((glare_down_kernel<true, false>), grid, dim3(GL_T), 0, nullptr, A);
        else hipLaunchKernelGGL((glare_down_kernel<false, false>), grid, dim3(GL_T), 0, nullptr, A);
    }
}

void launch_glare_down2(const GlareDown2Args &A) {
    const uint32_t w2 = ((A.sw + 1u) / 2u + 1u) / 2u, h2 = ((A.sh + 1u) / 2u + 1u) / 2u;
    const dim3 grid((w2 + GL_2X - 1) / GL_2X, (h2 + GL_2Y - 1) / GL_2Y);
    hipLaunchKernelGGL(glare_down2_kernel, grid, dim3(GL_T), 0, nullptr, A);
}

void launch_glare_up(const GlareUpArgs &A) {
    const dim3 grid((A.w + GL_PX - 1) / GL_PX, (A.h + GL_PY - 1) / GL_PY);
    hipLaunchKernelGGL(glare_up_kernel, grid, dim3(GL_T), 0, nullptr, A);
}

void launch_glare_composite(const GlareCompositeArgs &A) {
    const dim3 grid((A.w + GL_PX - 1) / GL_PX, (A.h + GL_PY - 1) / GL_PY);
    hipLaunchKernelGGL(glare_composite_kernel, grid, dim3(GL_T), 0, nullptr, A);
}

void launch_glare_tail(const GlareTailArgs &A) {
    hipLaunchKernelGGL(glare_tail_kernel, dim3(3), dim3(GL_TAIL_T), 0, nullptr, A);
}
