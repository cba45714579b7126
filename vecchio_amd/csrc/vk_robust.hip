// vk_robust.hip — the kernels behind vk_robust_* (include/vecchio_amd.h): a finished path batch added to a frame of K bucketed sums per
// pixel, and the frame's robust resolve.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the handle and
// the argument checks stay in vk_api.hip, which calls the launchers at the end of this file.
//
// State, per accumulator (vk_api.hip vk_robust): per pixel K cells of four 64-bit two's-complement words — the sums of r, g, b in 2^-26
// units and the count —, [pixel][bucket], 32 K bytes a pixel, and one record of four counters kept in stripes (vk_splat.h).  Every sum is
// an integer add: nothing depends on the order of the lanes or on how a batch was cut.
#include <hip/hip_runtime.h>

#include "vk_emit.h"
#include "vk_robust.h"

namespace {

constexpr int ROBUST_T = 256;                          // 4 waves a workgroup

}  // namespace

// robust_deposit_kernel: one lane per started id of a batch with nothing live; every id below n is a candidate, from its result.  The
// film's rule (vk_kernels.h deposit_lane) word for word: a candidate retired as MISS, ENDED or CULLED whose state's pixel lies in the
// frame is ours, everything else is skipped and touches nothing; one of ours with a non-finite acc is dropped, the others are converted
// as a film converts them.  The target is bucket state.sample % K of pixel state.pixel: a deposited result adds its three fixed values
// and 1 to the count, a dropped one 1 to the count only.  The four counters are ballots: one atomic per wave and non-zero counter, on
// the wave's stripe of the record — no lane leaves before them.  Everything else is a 64-bit atomic on global memory (the PLAIN form):
// after vk_film_emit with n_samples <= K no two lanes of a window share a cell, and a pixel's lanes cover consecutive cells.
__global__ __launch_bounds__(ROBUST_T) void robust_deposit_kernel(RobustDepositArgs A) {
    const uint32_t i = blockIdx.x * ROBUST_T + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = i < A.n;
    uint32_t status = (uint32_t)VK_SHADE_BAD_HIT;
    uint4 s1 = make_uint4(0u, 0u, 0u, 0u), s2 = s1;
    if (in) { status = A.result_status[i]; s1 = A.result_state[(size_t)i * 3u + 1u]; s2 = A.result_state[(size_t)i * 3u + 2u]; }
    const float ax = __uint_as_float(s1.x), ay = __uint_as_float(s1.y), az = __uint_as_float(s1.z);
    const bool retired = status == (uint32_t)VK_SHADE_MISS || status == (uint32_t)VK_SHADE_ENDED || status == (uint32_t)VK_PATHS_CULLED;
    const bool ours = in && retired && s2.z < A.n_pixels;
    const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az);
    const float big = fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az));
    const bool large = big > ACCUM_SMALL;
    const bool dep = ours && finite;
    const unsigned long long m_dep = __ballot(dep), m_drop = __ballot(ours && !finite);
    const unsigned long long m_clamp = __ballot(dep && large && big > A.accum_clamp), m_skip = __ballot(in && !ours);
    if (lane == 0u) {
        unsigned long long *c = A.counters + (size_t)((i >> 6) & (SPLAT_STRIPES - 1u)) * SPLAT_STRIPE_WORDS;      // the wave's stripe
        if (m_dep) atomicAdd(c + 0, (unsigned long long)__popcll(m_dep));
        if (m_drop) atomicAdd(c + 1, (unsigned long long)__popcll(m_drop));
        if (m_clamp) atomicAdd(c + 2, (unsigned long long)__popcll(m_clamp));
        if (m_skip) atomicAdd(c + 3, (unsigned long long)__popcll(m_skip));
    }
    if (!ours) return;                                 // (s2.z < n_pixels from here on: the cell lies inside the state)
    unsigned long long *cell = A.sums + ((size_t)s2.z * A.buckets + (size_t)(s2.w % A.buckets)) * 4u;
    if (dep) {
        unsigned long long fx, fy, fz;
        if (!large) {
            fx = (unsigned long long)to_fixed_small(ax); fy = (unsigned long long)to_fixed_small(ay); fz = (unsigned long long)to_fixed_small(az);
        } else {
            fx = (unsigned long long)to_fixed(ax, A.accum_clamp); fy = (unsigned long long)to_fixed(ay, A.accum_clamp);
            fz = (unsigned long long)to_fixed(az, A.accum_clamp);
        }
        atomicAdd(cell + 0, fx); atomicAdd(cell + 1, fy); atomicAdd(cell + 2, fz);
    }
    atomicAdd(cell + 3, 1ull);
}

// robust_resolve_kernel<K>: one lane per pixel, its K cells read once into registers and resolved by vk_robust.h's robust_resolve_pixel;
// rgb and, where asked for, the standard error in vk_render's f32 layout
template <int K>
__global__ __launch_bounds__(ROBUST_T) void robust_resolve_kernel(RobustResolveArgs A) {
    const uint32_t pix = blockIdx.x * ROBUST_T + threadIdx.x;
    if (pix >= A.n_pixels) return;
    float rgb[3], se[3];
    robust_resolve_pixel<K>(A.sums + (size_t)pix * K, A.mode, A.trim, rgb, se);
    float *o = A.rgb + (size_t)pix * 3u;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    if (A.se) {
        float *e = A.se + (size_t)pix * 3u;
        e[0] = se[0]; e[1] = se[1]; e[2] = se[2];
    }
}

// ---- the launchers (vk_robust.h): null stream, current device; sizes > 0 are the caller's to ensure
void launch_robust_deposit(const RobustDepositArgs &A) {
    hipLaunchKernelGGL(robust_deposit_kernel, dim3((A.n + ROBUST_T - 1) / ROBUST_T), dim3(ROBUST_T), 0, nullptr, A);
}

namespace {

template <int K>
void launch_resolve_k(const RobustResolveArgs &A) {
    hipLaunchKernelGGL(robust_resolve_kernel<K>, dim3((A.n_pixels + ROBUST_T - 1) / ROBUST_T), dim3(ROBUST_T), 0, nullptr, A);
}

}  // namespace

void launch_robust_resolve(const RobustResolveArgs &A, uint32_t buckets) {
    switch (buckets) {
        case 2: launch_resolve_k<2>(A); break;
        case 3: launch_resolve_k<3>(A); break;
        case 4: launch_resolve_k<4>(A); break;
        case 5: launch_resolve_k<5>(A); break;
        case 6: launch_resolve_k<6>(A); break;
        case 7: launch_resolve_k<7>(A); break;
        case 8: launch_resolve_k<8>(A); break;
        case 9: launch_resolve_k<9>(A); break;
        case 10: launch_resolve_k<10>(A); break;
        case 11: launch_resolve_k<11>(A); break;
        case 12: launch_resolve_k<12>(A); break;
        case 13: launch_resolve_k<13>(A); break;
        case 14: launch_resolve_k<14>(A); break;
        case 15: launch_resolve_k<15>(A); break;
        case 16: launch_resolve_k<16>(A); break;
        default: break;                                // (vk_api.hip admits 2..16 only)
    }
}
