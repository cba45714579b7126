// vk_robust.h — the kernels of vk_robust.hip as vk_api.hip sees them: their argument records and one thin launcher each (null stream,
// current device; the caller checks hipGetLastError).  The per-pixel resolve of a K-bucket table — the ordering, G, the trim, the kept
// sums and the standard error — is host-and-device: tests/emu/emu_robust.cpp builds it with g++.  The definition is
// include/vecchio_amd.h's ("robust film"); everything here is f32 and built without contraction.
#ifndef VK_ROBUST_H
#define VK_ROBUST_H

#include <stdint.h>

#include "vk_math.h"        // VK_HD
#include "vk_splat.h"       // the counter record's striping (SPLAT_STRIPES, SPLAT_STRIPE_WORDS) and the reason for it

enum : uint32_t { ROBUST_MEAN = 0u, ROBUST_TRIM = 1u, ROBUST_GINI = 2u };     // = VK_ROBUST_*
constexpr uint32_t ROBUST_MIN_BUCKETS = 2u, ROBUST_MAX_BUCKETS = 16u, ROBUST_COUNTERS = 4u;
constexpr uint64_t ROBUST_MAX_CELLS = 1ull << 27;      // width * height * K

// One bucket of one pixel: the sums of r, g, b in 2^-26 units and the count, two's complement.  The device layout is [pixel][bucket]
// (DESIGN.md "Robust film"): a pixel's table is K consecutive cells.
struct alignas(32) RobustCell {
    long long v[4];
};

#if defined(__HIPCC__) || defined(__HIP__)
#define VK_ROBUST_UNROLL _Pragma("unroll")
#else
#define VK_ROBUST_UNROLL
#endif

// The resolve of one pixel's table (include/vecchio_amd.h "robust film", steps 1 to 7).  Every array is indexed by unrolled loop counters
// only: on the device the table lives in registers for every K.  The order of the non-empty buckets is kept as a RANK per bucket — the
// number of non-empty buckets that come before it, by Y and then by index — and "bucket i of the order" is a select over the buckets:
// K^2 compares and selects, nothing beside the 32 K bytes the pixel reads.  The integer sums of the kept set need no order.
template <int K>
VK_HD void robust_resolve_pixel(const RobustCell *tab, uint32_t mode, uint32_t trim, float rgb[3], float se[3]) {
    const float inv_scale = 1.0f / 67108864.0f;      // 2^-26 (vk_emit.h ACCUM_SCALE)
    float Y[K], mr[K], mg[K], mb[K];
    bool ne[K];
    uint32_t j = 0u;
    VK_ROBUST_UNROLL
    for (int b = 0; b < K; b++) {
        const long long cnt = tab[b].v[3];
        ne[b] = cnt > 0;
        const float n = (float)cnt;
        mr[b] = ne[b] ? ((float)tab[b].v[0] * inv_scale) / n : 0.0f;
        mg[b] = ne[b] ? ((float)tab[b].v[1] * inv_scale) / n : 0.0f;
        mb[b] = ne[b] ? ((float)tab[b].v[2] * inv_scale) / n : 0.0f;
        Y[b] = (0.2126f * mr[b] + 0.7152f * mg[b]) + 0.0722f * mb[b];
        j += ne[b] ? 1u : 0u;
    }
    uint32_t rank[K];
    VK_ROBUST_UNROLL
    for (int b = 0; b < K; b++) {
        uint32_t r = 0u;
        VK_ROBUST_UNROLL
        for (int o = 0; o < K; o++) {
            if (o == b) continue;
            const bool before = Y[o] < Y[b] || (Y[o] == Y[b] && o < b);
            r += ne[o] && before ? 1u : 0u;
        }
        rank[b] = ne[b] ? r : 0xFFFFFFFFu;          // (an empty bucket has no place in the order)
    }
    // the order: oy[i] = Y_(i+1) and its means, for i < j
    float oy[K], or_[K], og[K], ob[K];
    VK_ROBUST_UNROLL
    for (int i = 0; i < K; i++) {
        float y = 0.0f, r = 0.0f, g = 0.0f, bl = 0.0f;
        VK_ROBUST_UNROLL
        for (int b = 0; b < K; b++) {
            const bool here = rank[b] == (uint32_t)i;
            y = here ? Y[b] : y; r = here ? mr[b] : r; g = here ? mg[b] : g; bl = here ? mb[b] : bl;
        }
        oy[i] = y; or_[i] = r; og[i] = g; ob[i] = bl;
    }
    const uint32_t tmax = j < 2u ? 0u : (j - 2u) / 2u;
    uint32_t t = 0u;
    if (mode == ROBUST_TRIM) {
        t = trim < tmax ? trim : tmax;
    } else if (mode == ROBUST_GINI) {
        float num = 0.0f, s = 0.0f;
        VK_ROBUST_UNROLL
        for (int i = 0; i < K; i++) {
            if ((uint32_t)i < j) {
                num = num + (float)(2 * (i + 1) - (int)j - 1) * oy[i];
                s = s + oy[i];
            }
        }
        const float G = (oy[0] >= 0.0f && s > 0.0f) ? num / ((float)j * s) : 0.0f;
        const float h = (G * (float)j) * 0.5f;
        // (h < 1, a G that rounding left below 0 included, trims nothing: the cast is taken of values >= 1 only)
        const uint32_t tg = h >= 1.0f ? (uint32_t)floorf(h) : 0u;
        t = tg < tmax ? tg : tmax;
    }
    const uint32_t hi = j - t, q = j - 2u * t;       // the kept ranks are t .. hi - 1 (j = 0: none)
    unsigned long long sr = 0ull, sg = 0ull, sb = 0ull, sn = 0ull;     // (unsigned: the sums wrap as two's complement does)
    VK_ROBUST_UNROLL
    for (int b = 0; b < K; b++) {
        const bool kept = ne[b] && rank[b] >= t && rank[b] < hi;
        sr += kept ? (unsigned long long)tab[b].v[0] : 0ull;
        sg += kept ? (unsigned long long)tab[b].v[1] : 0ull;
        sb += kept ? (unsigned long long)tab[b].v[2] : 0ull;
        sn += kept ? (unsigned long long)tab[b].v[3] : 0ull;
    }
    if (j == 0u) {
        rgb[0] = rgb[1] = rgb[2] = 0.0f;
        se[0] = se[1] = se[2] = 0.0f;
        return;
    }
    const float n = (float)(long long)sn;
    rgb[0] = ((float)(long long)sr * inv_scale) / n;
    rgb[1] = ((float)(long long)sg * inv_scale) / n;
    rgb[2] = ((float)(long long)sb * inv_scale) / n;
    if (q < 2u) {
        se[0] = se[1] = se[2] = 0.0f;
        return;
    }
    float Mr = 0.0f, Mg = 0.0f, Mb = 0.0f;
    VK_ROBUST_UNROLL
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i >= t && (uint32_t)i < hi) { Mr = Mr + or_[i]; Mg = Mg + og[i]; Mb = Mb + ob[i]; }
    }
    Mr = Mr / (float)q; Mg = Mg / (float)q; Mb = Mb / (float)q;
    float er = 0.0f, eg = 0.0f, eb = 0.0f;
    VK_ROBUST_UNROLL
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i >= t && (uint32_t)i < hi) {
            er = er + (or_[i] - Mr) * (or_[i] - Mr);
            eg = eg + (og[i] - Mg) * (og[i] - Mg);
            eb = eb + (ob[i] - Mb) * (ob[i] - Mb);
        }
    }
    const float d = (float)(q * (q - 1u));
    se[0] = sqrtf(er / d); se[1] = sqrtf(eg / d); se[2] = sqrtf(eb / d);
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// robust_deposit_kernel: one lane per started id of a finished batch
struct RobustDepositArgs {
    const uint4 *result_state;     // vk_path_state[n]
    const uint32_t *result_status; // [n]
    unsigned long long *sums;      // [n_pixels][buckets] cells of r, g, b, count
    unsigned long long *counters;  // [SPLAT_STRIPES][SPLAT_STRIPE_WORDS]: deposited, dropped, clamped, skipped in each
    uint32_t n, n_pixels, buckets;
    float accum_clamp;             // accum_clamp_for(samples_per_pixel)
};
// robust_resolve_kernel<K>: one lane per pixel
struct RobustResolveArgs {
    const RobustCell *sums;        // [n_pixels][K]
    float *rgb;                    // [n_pixels * 3]
    float *se;                     // [n_pixels * 3], or null
    uint32_t n_pixels, mode, trim;
};

void launch_robust_deposit(const RobustDepositArgs &A);
void launch_robust_resolve(const RobustResolveArgs &A, uint32_t buckets);      // buckets in 2..16
#endif

#endif
