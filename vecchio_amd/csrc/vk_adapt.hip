// vk_adapt.hip — the kernels behind vk_adapt_* (include/vecchio_amd.h): a film's error moments, the judge of its 8x8 tiles and the
// regenerating run over the pixels of the tiles still active.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the
// C ABI, the handles and the argument checks stay in vk_api.hip, which calls the launchers at the end of this file.
//
// State, per film (vk_api.hip AdaptState): prev = the sums at the last close, m2 = the batch-means moment sum_j n_j m_j^2, per tile
// tile_n (0 = active, else the count it froze with) and tile_k (its closes), the ascending list of the active tiles and its pixel prefix.
// Everything here is integer or unfused double arithmetic in a fixed order: nothing depends on how workgroups are scheduled.
#include <hip/hip_runtime.h>

#include "vk_emit.h"
#include "vk_adapt.h"

namespace {

constexpr int ADAPT_T = 256;           // 4 waves a workgroup
constexpr uint32_t ADAPT_SCAN_T = 1024u;   // tiles per workgroup of the list's two passes

__device__ __forceinline__ uint32_t tile_pixels(uint32_t t, uint32_t width, uint32_t height, uint32_t tiles_x) {
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t w = width - 8u * tx, h = height - 8u * ty;
    return (w < 8u ? w : 8u) * (h < 8u ? h : 8u);
}

// inclusive sum over the lanes of a wave (integers: exact in any order)
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

}  // namespace

// The top-up of a tile run.  adapt_locate gives the pixel and the sample of path first + j; the path is then vk_film_emit's for that
// (pixel, sample): start_camera_path on the one-pixel, one-sample window there, with the run's number as the id.
__global__ __launch_bounds__(ADAPT_T) void adapt_emit_kernel(AdaptEmitArgs A) {
    const uint32_t j = blockIdx.x * ADAPT_T + threadIdx.x;
    if (j >= A.m) return;
    const uint32_t q = A.first + j;
    uint32_t x, y, k;
    adapt_locate(A.T, A.n_samples, q, x, y, k);
    const EmitWindow W{x, y, 1u, A.first_sample + k, 1u};
    const size_t slot = (size_t)A.slot0 + j;
    start_camera_path(A.C, W, 0u, slot, A.rays, A.states, A.ids);
    A.ids[slot] = q;
}

__global__ __launch_bounds__(ADAPT_T) void adapt_sequence_kernel(AdaptSequenceArgs A) {
    const uint32_t j = blockIdx.x * ADAPT_T + threadIdx.x;
    if (j >= A.m) return;
    uint32_t x, y, k;
    A.pixel_out[j] = adapt_locate(A.T, A.n_samples, A.first + j, x, y, k);
    A.sample_out[j] = A.first_sample + k;
}

// A close: one wave per active tile, one lane per pixel (lane = 8 * row + column: a tile row's eight lanes touch 192 contiguous bytes of
// sums, prev and m2).  The fold is accumulate_resolve_kernel's, with the window's sum taken as sums - prev: w = sums - prev, prev = sums,
// s = (double)w / 2^26, m2 += s * s / n.  Then, where the rule may freeze (gate), adaptive_judge_kernel's vote at (done, steps): lanes
// outside the image do not vote, a tile whose pixels have all converged is frozen at (done, steps).  The counts of what is left come
// from the list's rebuild behind this launch: no atomic here.
__global__ __launch_bounds__(ADAPT_T) void adapt_close_kernel(AdaptCloseArgs A) {
    const uint32_t a = (blockIdx.x * ADAPT_T + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (a >= A.n_active) return;                               // (uniform per wave)
    const uint32_t t = A.list[a];
    const uint32_t ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
    const uint32_t px = tx * TILE + (lane & 7u), py = ty * TILE + (lane >> 3);
    const bool inside = px < A.width && py < A.height;
    bool conv = true;
    if (inside) {
        const double N = (double)A.done, k = (double)A.steps, at = (double)A.abs_tol, rt = (double)A.rel_tol;
        for (int c = 0; c < 3; c++) {
            const size_t i = ((size_t)py * A.width + px) * 3 + c;
            const long long r = A.sums[i], w = r - A.prev[i];
            A.prev[i] = r;
            const double s = (double)w * (1.0 / (double)ACCUM_SCALE);
            const double m = A.m2[i] + s * s / (double)A.window;
            A.m2[i] = m;
            if (A.gate) {
                const double mean = (double)r / (double)ACCUM_SCALE / N;
                const double v = (m - N * mean * mean) / ((k - 1.0) * N);
                const double tol = at + rt * fabs(mean);
                conv = conv && v <= tol * tol;
            }
        }
    }
    const unsigned long long conv_mask = __ballot(conv);
    if (lane == 0 && A.gate && conv_mask == ~0ull) { A.tile_n[t] = A.done; A.tile_k[t] = A.steps; }
}

// The list, 1: the active tiles and their in-image pixels per block of 1024 tiles.
__global__ __launch_bounds__(ADAPT_SCAN_T) void adapt_count_kernel(AdaptListArgs A) {
    __shared__ uint32_t wt[16], wp[16];
    const uint32_t t = blockIdx.x * ADAPT_SCAN_T + threadIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool act = t < A.tiles && A.tile_n[t] == 0u;
    const uint32_t px = wave_scan(act ? tile_pixels(t, A.width, A.height, A.tiles_x) : 0u, lane);
    const unsigned long long m = __ballot(act);
    if (lane == 63u) { wt[w] = (uint32_t)__popcll(m); wp[w] = px; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t st = 0, sp = 0;
        for (int k = 0; k < 16; k++) { st += wt[k]; sp += wp[k]; }
        A.block_tiles[blockIdx.x] = st; A.block_px[blockIdx.x] = sp;
    }
}

// The list, 2: every block adds up the counts of the blocks before it and writes its active tiles, in ascending order, behind them with
// the pixels before each (an integer scan: the same list on every run); the last block writes the totals — prefix[n_active] and the
// record the host reads.
__global__ __launch_bounds__(ADAPT_SCAN_T) void adapt_scatter_kernel(AdaptListArgs A) {
    __shared__ uint32_t part_t[ADAPT_SCAN_T], part_p[ADAPT_SCAN_T];
    __shared__ uint32_t wt[16], wp[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t st = 0, sp = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += ADAPT_SCAN_T) { st += A.block_tiles[b]; sp += A.block_px[b]; }
    part_t[threadIdx.x] = st; part_p[threadIdx.x] = sp;
    const uint32_t t = blockIdx.x * ADAPT_SCAN_T + threadIdx.x;
    const bool act = t < A.tiles && A.tile_n[t] == 0u;
    const uint32_t mine = act ? tile_pixels(t, A.width, A.height, A.tiles_x) : 0u;
    const uint32_t px = wave_scan(mine, lane);                 // inclusive
    const unsigned long long m = __ballot(act);
    if (lane == 63u) { wt[w] = (uint32_t)__popcll(m); wp[w] = px; }
    __syncthreads();
    for (uint32_t h = ADAPT_SCAN_T / 2u; h > 0u; h >>= 1) {
        if (threadIdx.x < h) { part_t[threadIdx.x] += part_t[threadIdx.x + h]; part_p[threadIdx.x] += part_p[threadIdx.x + h]; }
        __syncthreads();
    }
    uint32_t base_t = part_t[0], base_p = part_p[0];
    for (uint32_t k = 0; k < w; k++) { base_t += wt[k]; base_p += wp[k]; }
    if (act) {
        const uint32_t at = base_t + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        A.list[at] = t; A.prefix[at] = base_p + (px - mine);
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) {
        uint32_t n = part_t[0], p = part_p[0];
        for (int k = 0; k < 16; k++) { n += wt[k]; p += wp[k]; }
        A.prefix[n] = p;
        A.record[0] = n; A.record[1] = p;
    }
}

// vk_film_resolve's arithmetic on the sums of the last close, every pixel over its tile's own count
__global__ __launch_bounds__(ADAPT_T) void adapt_resolve_kernel(AdaptImageArgs A) {
    const uint32_t pix = blockIdx.x * ADAPT_T + threadIdx.x;
    if (pix >= A.width * A.height) return;
    const uint32_t x = pix % A.width, y = pix / A.width;
    const uint32_t tn = A.tile_n[(y / TILE) * A.tiles_x + x / TILE];
    const float n = (float)(tn ? tn : A.done);
    const long long *a = A.prev + (size_t)pix * 3;
    const float inv_scale = 1.0f / ACCUM_SCALE;
    A.out[(size_t)pix * 3 + 0] = ((float)a[0] * inv_scale) / n;
    A.out[(size_t)pix * 3 + 1] = ((float)a[1] * inv_scale) / n;
    A.out[(size_t)pix * 3 + 2] = ((float)a[2] * inv_scale) / n;
}

// progress_stderr_kernel's expression, in its order, with each tile's own N and k
__global__ __launch_bounds__(ADAPT_T) void adapt_stderr_kernel(AdaptImageArgs A) {
    const uint32_t pix = blockIdx.x * ADAPT_T + threadIdx.x;
    if (pix >= A.width * A.height) return;
    const uint32_t x = pix % A.width, y = pix / A.width;
    const uint32_t t = (y / TILE) * A.tiles_x + x / TILE;
    const uint32_t tn = A.tile_n[t];
    const double N = (double)(tn ? tn : A.done), k = (double)(tn ? A.tile_k[t] : A.steps);
    for (int c = 0; c < 3; c++) {
        const size_t i = (size_t)pix * 3 + c;
        const double mean = (double)A.prev[i] / (double)ACCUM_SCALE / N;
        const double v = (A.m2[i] - N * mean * mean) / ((k - 1.0) * N);
        A.out[i] = (float)sqrt(v > 0.0 ? v : 0.0);
    }
}

// ---- the launchers (vk_adapt.h): null stream, current device; sizes > 0 are the caller's to ensure
void launch_adapt_emit(const AdaptEmitArgs &A) {
    hipLaunchKernelGGL(adapt_emit_kernel, dim3((A.m + ADAPT_T - 1) / ADAPT_T), dim3(ADAPT_T), 0, nullptr, A);
}
void launch_adapt_sequence(const AdaptSequenceArgs &A) {
    hipLaunchKernelGGL(adapt_sequence_kernel, dim3((A.m + ADAPT_T - 1) / ADAPT_T), dim3(ADAPT_T), 0, nullptr, A);
}
void launch_adapt_close(const AdaptCloseArgs &A) {
    hipLaunchKernelGGL(adapt_close_kernel, dim3((A.n_active + 3u) / 4u), dim3(ADAPT_T), 0, nullptr, A);
}
void launch_adapt_list(const AdaptListArgs &A) {
    const uint32_t nb = (A.tiles + ADAPT_SCAN_T - 1u) / ADAPT_SCAN_T;
    hipLaunchKernelGGL(adapt_count_kernel, dim3(nb), dim3(ADAPT_SCAN_T), 0, nullptr, A);
    hipLaunchKernelGGL(adapt_scatter_kernel, dim3(nb), dim3(ADAPT_SCAN_T), 0, nullptr, A);
}
void launch_adapt_resolve(const AdaptImageArgs &A) {
    const uint32_t n = A.width * A.height;
    hipLaunchKernelGGL(adapt_resolve_kernel, dim3((n + ADAPT_T - 1) / ADAPT_T), dim3(ADAPT_T), 0, nullptr, A);
}
void launch_adapt_stderr(const AdaptImageArgs &A) {
    const uint32_t n = A.width * A.height;
    hipLaunchKernelGGL(adapt_stderr_kernel, dim3((n + ADAPT_T - 1) / ADAPT_T), dim3(ADAPT_T), 0, nullptr, A);
}
