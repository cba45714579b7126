// vk_splat.hip — the kernels behind vk_splat_* (include/vecchio_amd.h): a finished path batch splatted into a filtered frame, and the
// frame's resolve.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the handle and the argument checks
// stay in vk_api.hip, which calls the launchers at the end of this file.
//
// State, per accumulator (vk_api.hip vk_splat): per pixel four 64-bit two's-complement sums in 2^-26 units, interleaved {r, g, b, w} —
// 32 bytes, a row of pixels contiguous — and one record of five counters, kept in stripes (vk_splat.h).  Every sum is an integer add: nothing depends on the order of
// the lanes, on how a batch was cut or on the kernel's form.
#include <hip/hip_runtime.h>

#include "vk_emit.h"
#include "vk_splat.h"

namespace {

constexpr int SPLAT_T = 256;                          // 4 waves a workgroup
// The TILED form's LDS tile: the anchor row of the workgroup's first depositing lane +-2, and the columns from that anchor's - 2 on: one
// column per lane plus the halo of 2 on either side.  (256 + 4) x 5 x 32 B = 41600 B: three workgroups a CU.
constexpr int SPLAT_TILE_W = SPLAT_T + 4, SPLAT_TILE_H = 5;
constexpr int SPLAT_TILE_WORDS = SPLAT_TILE_W * SPLAT_TILE_H * 4;

// the four fixed-point values of weight w on a clamped sample (vk_emit.h's split: |w| <= 1, so |w a| stays inside the small path's range
// where the sample did)
__device__ __forceinline__ void splat_fixed(float w, float ax, float ay, float az, bool large, float clampv, unsigned long long v[4]) {
    if (!large) {
        v[0] = (unsigned long long)to_fixed_small(w * ax); v[1] = (unsigned long long)to_fixed_small(w * ay);
        v[2] = (unsigned long long)to_fixed_small(w * az);
    } else {
        v[0] = (unsigned long long)to_fixed(w * ax, clampv); v[1] = (unsigned long long)to_fixed(w * ay, clampv);
        v[2] = (unsigned long long)to_fixed(w * az, clampv);
    }
    v[3] = (unsigned long long)to_fixed_small(w);
}

// sum over the lanes of a wave, in every lane (integers: exact in any order)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

// splat_deposit_kernel<TILED>: one lane per started id of a batch with nothing live; every id below n is a candidate, from its result.
// A candidate retired as MISS, ENDED or CULLED whose position lies in the frame is placed (everything else: skipped); a placed one with
// a non-finite acc is dropped; the others are clamped as a film clamps them and added, weight by weight, to the pixels of their
// footprint (splat_weights).  The five counters are ballots and one wave sum: one atomic per wave and non-zero counter, on the wave's
// stripe of the record — no lane leaves before them.
//   TILED = false (PLAIN): every (pixel, sum) is a 64-bit atomic on global memory.
//   TILED = true: the workgroup's lanes are consecutive ids — after vk_film_emit the samples of consecutive pixels of a row, whose
//     footprints overlap.  They add into an LDS tile with 64-bit LDS atomics where the target lies inside it and straight to global
//     memory where it does not (row wraps, the caller's own pixel order, positions); behind a barrier the tile's non-zero values go out
//     by global atomics, lanes running along a row: a wave-instruction covers contiguous 32-byte pixels.
template <bool TILED>
__global__ __launch_bounds__(SPLAT_T) void splat_deposit_kernel(SplatDepositArgs A) {
    __shared__ unsigned long long tile[TILED ? SPLAT_TILE_WORDS : 1];
    __shared__ uint32_t wave_first[TILED ? 4 : 1];     // per wave: the anchor pixel of its first depositing lane, or ~0
    const uint32_t i = blockIdx.x * SPLAT_T + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = i < A.n;
    uint32_t status = (uint32_t)VK_SHADE_BAD_HIT;
    uint4 s1 = make_uint4(0u, 0u, 0u, 0u), s2 = s1;
    if (in) { status = A.result_status[i]; s1 = A.result_state[(size_t)i * 3u + 1u]; s2 = A.result_state[(size_t)i * 3u + 2u]; }
    const bool retired = status == (uint32_t)VK_SHADE_MISS || status == (uint32_t)VK_SHADE_ENDED || status == (uint32_t)VK_PATHS_CULLED;
    uint32_t ix = 0u, iy = 0u;
    float fx = 0.0f, fy = 0.0f;
    bool placed = false;
    if (in && retired) {
        if (A.positions) {
            const float2 p = A.positions[i];
            placed = splat_position_given(p.x, p.y, A.width, A.height, ix, iy, fx, fy);
        } else {
            placed = splat_position_of_state(((uint64_t)s2.y << 32) | (uint64_t)s2.x, s2.z, s2.w, A.width, A.height, ix, iy, fx, fy);
        }
    }
    float ax = __uint_as_float(s1.x), ay = __uint_as_float(s1.y), az = __uint_as_float(s1.z);
    const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az);
    const float big = fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az));
    const bool large = big > ACCUM_SMALL;
    const bool dep = placed && finite;
    SplatFoot F;
    uint32_t contrib = 0u;
    if (dep) contrib = splat_weights(A.P, ix, fx, iy, fy, A.width, A.height, F);
    else F.mx = F.my = 0u;
    const unsigned long long m_dep = __ballot(dep), m_drop = __ballot(placed && !finite);
    const unsigned long long m_clamp = __ballot(dep && large && big > A.accum_clamp), m_skip = __ballot(in && !placed);
    const uint32_t n_contrib = wave_sum(contrib);
    if (lane == 0u) {
        unsigned long long *c = A.counters + (size_t)((i >> 6) & (SPLAT_STRIPES - 1u)) * SPLAT_STRIPE_WORDS;      // the wave's stripe
        if (m_dep) atomicAdd(c + 0, (unsigned long long)__popcll(m_dep));
        if (m_drop) atomicAdd(c + 1, (unsigned long long)__popcll(m_drop));
        if (m_clamp) atomicAdd(c + 2, (unsigned long long)__popcll(m_clamp));
        if (m_skip) atomicAdd(c + 3, (unsigned long long)__popcll(m_skip));
        if (n_contrib) atomicAdd(c + 4, (unsigned long long)n_contrib);
    }
    if (large) {
        ax = fminf(fmaxf(ax, -A.accum_clamp), A.accum_clamp); ay = fminf(fmaxf(ay, -A.accum_clamp), A.accum_clamp);
        az = fminf(fmaxf(az, -A.accum_clamp), A.accum_clamp);
    }
    int tx0 = 0, ty0 = 0;
    if (TILED) {
        // (every lane of the wave takes part in the shuffle: a lane that is masked off would hand over nothing)
        const uint32_t anchor = (uint32_t)__shfl((int)(iy * A.width + ix), m_dep ? __builtin_ctzll(m_dep) : 0, 64);
        if (lane == 0u) wave_first[threadIdx.x >> 6] = m_dep ? anchor : 0xFFFFFFFFu;
        for (int w = threadIdx.x; w < SPLAT_TILE_WORDS; w += SPLAT_T) tile[w] = 0ull;
        __syncthreads();
        uint32_t first = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 3; w >= 0; w--) if (wave_first[w] != 0xFFFFFFFFu) first = wave_first[w];
        if (first == 0xFFFFFFFFu) return;                           // (uniform: nothing to add in this workgroup)
        const uint32_t fy0 = first / A.width;
        tx0 = (int)(first - fy0 * A.width) - 2; ty0 = (int)fy0 - 2;
    }
#pragma unroll
    for (int ky = 0; ky < 5; ky++) {
#pragma unroll
        for (int kx = 0; kx < 5; kx++) {
            if (((F.my >> ky) & 1u) && ((F.mx >> kx) & 1u)) {       // inside the frame: 0 <= X < width, 0 <= Y < height
                const int X = (int)ix + kx - 2, Y = (int)iy + ky - 2;
                unsigned long long v[4];
                splat_fixed(F.wx[kx] * F.wy[ky], ax, ay, az, large, A.accum_clamp, v);
                bool local = false;
                if (TILED) {
                    const int lx = X - tx0, ly = Y - ty0;
                    local = lx >= 0 && lx < SPLAT_TILE_W && ly >= 0 && ly < SPLAT_TILE_H;
                    if (local) {
                        unsigned long long *t = tile + (ly * SPLAT_TILE_W + lx) * 4;
                        atomicAdd(t + 0, v[0]); atomicAdd(t + 1, v[1]); atomicAdd(t + 2, v[2]); atomicAdd(t + 3, v[3]);
                    }
                }
                if (!local) {
                    unsigned long long *g = A.sums + ((size_t)Y * A.width + (size_t)X) * 4u;
                    atomicAdd(g + 0, v[0]); atomicAdd(g + 1, v[1]); atomicAdd(g + 2, v[2]); atomicAdd(g + 3, v[3]);
                }
            }
        }
    }
    if (TILED) {
        __syncthreads();
        // (a non-zero value was added by a lane whose target lay inside the frame: its pixel is one)
        for (int c = threadIdx.x; c < SPLAT_TILE_W * SPLAT_TILE_H; c += SPLAT_T) {
            const int ly = c / SPLAT_TILE_W, lx = c - ly * SPLAT_TILE_W;
            const unsigned long long *t = tile + c * 4;
            const unsigned long long v0 = t[0], v1 = t[1], v2 = t[2], v3 = t[3];
            if ((v0 | v1 | v2 | v3) == 0ull) continue;
            unsigned long long *g = A.sums + ((size_t)(ty0 + ly) * A.width + (size_t)(tx0 + lx)) * 4u;
            if (v0) atomicAdd(g + 0, v0);
            if (v1) atomicAdd(g + 1, v1);
            if (v2) atomicAdd(g + 2, v2);
            if (v3) atomicAdd(g + 3, v3);
        }
    }
}

// rgb = w_sum > 0 ? ((float)c_sum * 2^-26) / ((float)w_sum * 2^-26) : 0, in vk_render's f32 layout
__global__ __launch_bounds__(SPLAT_T) void splat_resolve_kernel(SplatResolveArgs A) {
    const uint32_t pix = blockIdx.x * SPLAT_T + threadIdx.x;
    if (pix >= A.n_pixels) return;
    const long long *a = A.sums + (size_t)pix * 4u;
    const float inv_scale = 1.0f / ACCUM_SCALE;
    const long long ws = a[3];
    const float w = (float)ws * inv_scale;
    float *o = A.out + (size_t)pix * 3u;
    o[0] = ws > 0 ? ((float)a[0] * inv_scale) / w : 0.0f;
    o[1] = ws > 0 ? ((float)a[1] * inv_scale) / w : 0.0f;
    o[2] = ws > 0 ? ((float)a[2] * inv_scale) / w : 0.0f;
}

// ---- the launchers (vk_splat.h): null stream, current device; sizes > 0 are the caller's to ensure
void launch_splat_deposit(const SplatDepositArgs &A, bool tiled) {
    const dim3 grid((A.n + SPLAT_T - 1) / SPLAT_T);
    if (tiled) hipLaunchKernelGGL(splat_deposit_kernel<true>, grid, dim3(SPLAT_T), 0, nullptr, A);
    else hipLaunchKernelGGL(splat_deposit_kernel<false>, grid, dim3(SPLAT_T), 0, nullptr, A);
}
void launch_splat_resolve(const SplatResolveArgs &A) {
    hipLaunchKernelGGL(splat_resolve_kernel, dim3((A.n_pixels + SPLAT_T - 1) / SPLAT_T), dim3(SPLAT_T), 0, nullptr, A);
}
