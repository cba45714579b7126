// vk_nlm.hip — the kernels behind vk_nlm_* (include/vecchio_amd.h "non-local means"): the prepare pass into the handle's planes and the
// filter in its two forms.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the handle and the argument
// checks stay in vk_api.hip, which calls the launchers at the end of this file.
//
// The per-pixel code is vk_nlm.h's, shared with the host build of tests/emu.  Both forms add the same f32 values in the same order —
// a patch sum is rows first (i ascending), then the rows (j ascending) — so they agree bit for bit.
#include <hip/hip_runtime.h>

#include "vk_nlm.h"

namespace {

constexpr int NLM_T = 256;                             // 4 waves a workgroup
constexpr int NLM_PX = 64, NLM_PY = 4;                 // prepare and the PLAIN form: one wave per row of 64 pixels
constexpr int NLM_TX = 32, NLM_TY = 8;                 // the TILED form's tile: half a wave per row, so every LDS read of a half-wave is
                                                       // 32 consecutive dwords (ds_read_b32 banks per 32-lane half: no conflict)
constexpr int NLM_EW = NLM_TX + 2 * (int)NLM_MAX_F, NLM_EH = NLM_TY + 2 * (int)NLM_MAX_F;      // the pair plane: the tile and an F halo

}  // namespace

// nlm_prepare_kernel: one lane per pixel; a, I, V of the pixel and Vf from the 3x3 neighbours' V, recomputed from the inputs (nothing is
// read that another lane of this launch writes)
__global__ __launch_bounds__(NLM_T) void nlm_prepare_kernel(NlmPrepareArgs A) {
    const int x = (int)(blockIdx.x * NLM_PX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * NLM_PY + (threadIdx.x >> 6));
    const int w = (int)A.width, h = (int)A.height;
    if (x >= w || y >= h) return;
    const size_t n = (size_t)A.width * A.height, p = (size_t)y * A.width + (size_t)x;
    float I[3], V[3], Vf[3], a[3];
    nlm_prepare_pixel(A.color, A.stderr3, A.albedo, A.albedo_floor, w, h, x, y, I, V, Vf, a);
#pragma unroll
    for (int c = 0; c < 3; c++) { A.I[c * n + p] = I[c]; A.V[c * n + p] = V[c]; A.Vf[c * n + p] = Vf[c]; A.a[c * n + p] = a[c]; }
}

// nlm_filter_kernel<FORM, HALO>.
//
// PLAIN (HALO 0): one lane per pixel, the definition straight from global memory (nlm_filter_pixel): the yardstick and the fallback.
//
// TILED: a workgroup owns NLM_TX x NLM_TY pixels.  It stages I and Vf of the tile and a halo of R + F <= HALO pixels in LDS, six planes,
// a slot outside the image stored as invalid (Vf_r = -1), so the loops below test no bounds.  Per offset o: (1) e and c of the pair (a, a +
// o) once for every pixel a of the tile and an F halo, into sE / sC; (2) the row sums over i once per pixel of the tile's columns and
// its rows with an F halo, into sR / sM; (3) every lane sums its 2F + 1 rows and accumulates W, J, U in registers.  Two barriers an
// offset: (2) and (3) of one offset and (1) of the next lie between the same pair.
template <uint32_t FORM, int HALO>
__global__ __launch_bounds__(NLM_T) void nlm_filter_kernel(NlmFilterArgs A) {
    const NlmPlanes &P = A.P;
    const int w = (int)P.width, h = (int)P.height;
    const size_t n = (size_t)P.width * P.height;
    if constexpr (FORM == NLM_FORM_PLAIN) {
        const int x = (int)(blockIdx.x * NLM_PX + (threadIdx.x & 63u)), y = (int)(blockIdx.y * NLM_PY + (threadIdx.x >> 6));
        if (x >= w || y >= h) return;
        const size_t p = (size_t)y * P.width + (size_t)x;
        float out[3], se[3];
        nlm_filter_pixel(P, x, y, A.R, A.F, A.alpha, A.kk, out, se);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A.out[p * 3 + c] = out[c];
            if (A.stderr3_out) A.stderr3_out[p * 3 + c] = se[c];
        }
    } else {
        constexpr int SLOTS = (NLM_TX + 2 * HALO) * (NLM_TY + 2 * HALO);
        __shared__ float sI[3][SLOTS], sVf[3][SLOTS];
        __shared__ float sE[NLM_EW * NLM_EH], sR[NLM_TX * NLM_EH];
        __shared__ uint32_t sC[NLM_EW * NLM_EH], sM[NLM_TX * NLM_EH];
        const int R = A.R, F = A.F, H = R + F;                       // H <= HALO: the launcher's to ensure
        const int cols = NLM_TX + 2 * H, rows = NLM_TY + 2 * H, ew = NLM_TX + 2 * F, eh = NLM_TY + 2 * F;
        const int x0 = (int)blockIdx.x * NLM_TX, y0 = (int)blockIdx.y * NLM_TY;
        const int tid = (int)threadIdx.x, tx = tid & (NLM_TX - 1), ty = tid / NLM_TX;
        for (int i = tid; i < rows * cols; i += NLM_T) {
            const int sy = i / cols, sx = i - sy * cols, gx = x0 - H + sx, gy = y0 - H + sy;
            const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
            const size_t g = in ? (size_t)gy * P.width + (size_t)gx : 0u;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                sI[c][i] = in ? P.I[c * n + g] : 0.0f;
                sVf[c][i] = in ? P.Vf[c * n + g] : (c == 0 ? -1.0f : 0.0f);
            }
        }
        __syncthreads();
        const int x = x0 + tx, y = y0 + ty;
        const int sp = (H + ty) * cols + (H + tx);                   // this lane's pixel in the staged planes
        const bool live = x < w && y < h && !(sVf[0][sp] < 0.0f);    // in the image and valid
        NlmSums s;
        nlm_sums_clear(s);
#pragma unroll 1
        for (int oy = -R; oy <= R; oy++) {
#pragma unroll 1
            for (int ox = -R; ox <= R; ox++) {
                const int sq = sp + oy * cols + ox;
                const bool take = live && !(sVf[0][sq] < 0.0f);
                float wgt = 1.0f;
                if (ox != 0 || oy != 0) {
                    // (1) the pair plane
                    for (int i = tid; i < ew * eh; i += NLM_T) {
                        const int ey = i / ew, ex = i - ey * ew;
                        const int sa = (H - F + ey) * cols + (H - F + ex), sb = sa + oy * cols + ox;
                        float e = 0.0f;
                        uint32_t c = 0u;
                        if (!(sVf[0][sa] < 0.0f) && !(sVf[0][sb] < 0.0f)) {
                            const float Ia[3] = {sI[0][sa], sI[1][sa], sI[2][sa]}, Ib[3] = {sI[0][sb], sI[1][sb], sI[2][sb]};
                            const float Va[3] = {sVf[0][sa], sVf[1][sa], sVf[2][sa]}, Vb[3] = {sVf[0][sb], sVf[1][sb], sVf[2][sb]};
                            e = nlm_pair(Ia, Va, Ib, Vb, A.alpha, A.kk);
                            c = 1u;
                        }
                        sE[i] = e; sC[i] = c;
                    }
                    __syncthreads();
                    // (2) the row sums, i ascending from 0
                    for (int i = tid; i < NLM_TX * eh; i += NLM_T) {
                        const int ry = i / NLM_TX, rx = i & (NLM_TX - 1);
                        const int at = ry * ew + rx;
                        float r = 0.0f;
                        uint32_t m = 0u;
                        for (int k = 0; k <= 2 * F; k++) { r += sE[at + k]; m += sC[at + k]; }
                        sR[i] = r; sM[i] = m;
                    }
                    __syncthreads();
                    // (3) the rows, j ascending from 0
                    float S = 0.0f;
                    uint32_t cnt = 0u;
                    for (int k = 0; k <= 2 * F; k++) { S += sR[(ty + k) * NLM_TX + tx]; cnt += sM[(ty + k) * NLM_TX + tx]; }
                    wgt = nlm_weight(S, take ? cnt : 1u);
                }
                if (take) {
                    const size_t q = (size_t)(y + oy) * P.width + (size_t)(x + ox);      // in the image: its staged slot is valid
                    const float Iq[3] = {sI[0][sq], sI[1][sq], sI[2][sq]}, Vq[3] = {P.V[q], P.V[n + q], P.V[2 * n + q]};
                    nlm_sums_add(s, wgt, Iq, Vq);
                }
            }
        }
        if (x >= w || y >= h) return;
        const size_t p = (size_t)y * P.width + (size_t)x;
        float out[3], se[3];
        if (live) {
            const float a[3] = {P.a[p], P.a[n + p], P.a[2 * n + p]};
            nlm_finish(s, a, out, se);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) { out[c] = P.I[c * n + p]; se[c] = P.V[c * n + p]; }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A.out[p * 3 + c] = out[c];
            if (A.stderr3_out) A.stderr3_out[p * 3 + c] = se[c];
        }
    }
}

// ---- the launchers (vk_nlm.h): null stream, current device; sizes > 0 and R, F in range are the caller's to ensure
void launch_nlm_prepare(const NlmPrepareArgs &A) {
    const dim3 grid((A.width + NLM_PX - 1) / NLM_PX, (A.height + NLM_PY - 1) / NLM_PY);
    hipLaunchKernelGGL(nlm_prepare_kernel, grid, dim3(NLM_T), 0, nullptr, A);
}

void launch_nlm_filter(const NlmFilterArgs &A, uint32_t form) {
    if (form == NLM_FORM_PLAIN) {
        const dim3 grid((A.P.width + NLM_PX - 1) / NLM_PX, (A.P.height + NLM_PY - 1) / NLM_PY);
        hipLaunchKernelGGL((nlm_filter_kernel<NLM_FORM_PLAIN, 0>), grid, dim3(NLM_T), 0, nullptr, A);
        return;
    }
    const dim3 grid((A.P.width + NLM_TX - 1) / NLM_TX, (A.P.height + NLM_TY - 1) / NLM_TY);
    if (A.R + A.F <= NLM_TILED_SMALL_HALO)
        hipLaunchKernelGGL((nlm_filter_kernel<NLM_FORM_TILED, NLM_TILED_SMALL_HALO>), grid, dim3(NLM_T), 0, nullptr, A);
    else
        hipLaunchKernelGGL((nlm_filter_kernel<NLM_FORM_TILED, NLM_TILED_LARGE_HALO>), grid, dim3(NLM_T), 0, nullptr, A);
}
