// vk_splat.h — the kernels of vk_splat.hip as vk_api.hip sees them: their argument records and one thin launcher each (null stream,
// current device; the caller checks hipGetLastError).  What decides a sample's footprint — the filter's coefficients, its position and
// splat_weights — is host-and-device: tests/emu/emu_splat.cpp builds it with g++.  The definition is include/vecchio_amd.h's
// ("reconstruction filters"); everything here is f32 and built without contraction.
#ifndef VK_SPLAT_H
#define VK_SPLAT_H

#include <stdint.h>

#include "vk_math.h"        // VK_HD, the sample streams

enum : uint32_t { SPLAT_BOX = 0u, SPLAT_TENT = 1u, SPLAT_MITCHELL = 2u };     // = VK_SPLAT_*
// the deposit's default form: the one measured faster on the majority of the report's rows (DESIGN.md "Reconstruction filters")
constexpr bool SPLAT_DEFAULT_TILED = true;
// The counter record is kept in stripes, SPLAT_STRIPE_WORDS 64-bit words (256 bytes) apart; a wave adds to the stripe of its own number
// and the host sums them.  Atomics on ONE word complete at about 88 per microsecond on this chip whatever issues them: a frame of 16.6 M
// paths is 259 200 waves, and their counter atomics on a single record took as long as everything else of the deposit together.
constexpr uint32_t SPLAT_STRIPES = 32u, SPLAT_STRIPE_WORDS = 32u, SPLAT_COUNTERS = 5u;

// A filter as the kernels take it: what the host computes once from vk_splat_params.  near/far: the Mitchell-Netravali cubic's
// coefficients on t < 1 (t^3, t^2, 1) and on 1 <= t < 2 (t^3, t^2, t, 1).
struct SplatFilter {
    uint32_t filter;
    float radius, inv_r, t_scale;      // 1 / radius; 2 * inv_r
    float p3, p2, p0;
    float q3, q2, q1, q0;
};

VK_HD SplatFilter splat_filter_for(uint32_t filter, float radius, float b, float c) {
    SplatFilter P;
    P.filter = filter; P.radius = radius; P.inv_r = 1.0f / radius; P.t_scale = 2.0f * P.inv_r;
    P.p3 = ((12.0f - 9.0f * b) - 6.0f * c) / 6.0f;
    P.p2 = ((-18.0f + 12.0f * b) + 6.0f * c) / 6.0f;
    P.p0 = (6.0f - 2.0f * b) / 6.0f;
    P.q3 = (-b - 6.0f * c) / 6.0f;
    P.q2 = (6.0f * b + 30.0f * c) / 6.0f;
    P.q1 = (-12.0f * b - 48.0f * c) / 6.0f;
    P.q0 = (8.0f * b + 24.0f * c) / 6.0f;
    return P;
}

// the filter's value at distance a = |d| >= 0 from the pixel's centre, on one axis (the caller has checked the support)
VK_HD float splat_w1(const SplatFilter &P, float a) {
    if (P.filter == SPLAT_BOX) return 1.0f;
    if (P.filter == SPLAT_TENT) return 1.0f - a * P.inv_r;
    const float t = a * P.t_scale;
    if (t < 1.0f) return ((P.p3 * t + P.p2) * t) * t + P.p0;
    return ((P.q3 * t + P.q2) * t + P.q1) * t + P.q0;
}

VK_HD bool splat_finite(float v) { return (vk::f32_bits(v) & 0x7F800000u) != 0x7F800000u; }

// A sample's position from its state: the anchor is the state's pixel, the offsets are draws 0 and 1 of the sample's stream — for a
// film's camera path the jitter its ray was generated with (vk_trace.h start_sample_core).  false: the pixel lies outside the frame.
VK_HD bool splat_position_of_state(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t width, uint32_t height, uint32_t &ix,
                                   uint32_t &iy, float &fx, float &fy) {
    if (pixel >= width * height) return false;
    iy = pixel / width; ix = pixel - iy * width;
    vk::Rng g = vk::rng_for_sample(seed, pixel, sample);
    fx = vk::gen_f32(g);
    fy = vk::gen_f32(g);
    return true;
}
// ... and from the caller's frame coordinates.  false: not finite, or the anchor lies outside the frame (-0.0 is pixel 0).
VK_HD bool splat_position_given(float px, float py, uint32_t width, uint32_t height, uint32_t &ix, uint32_t &iy, float &fx, float &fy) {
    if (!splat_finite(px) || !splat_finite(py)) return false;
    const float flx = floorf(px), fly = floorf(py);
    if (!(flx >= 0.0f && flx < (float)width && fly >= 0.0f && fly < (float)height)) return false;     // (extents <= 2^26: exact)
    ix = (uint32_t)flx; iy = (uint32_t)fly;
    fx = px - flx; fy = py - fly;
    return true;
}

// The footprint of a sample at (ix + fx, iy + fy): candidate k = -2 .. 2 of an axis is pixel ix + k at d = (fx - 0.5f) - (float)k from
// its centre, in support iff -radius <= d < radius.  Bit k + 2 of a mask: in support AND inside the frame; its weight is set then, 0
// otherwise.  The sample's weight on pixel (ix + kx, iy + ky) is wx[kx + 2] * wy[ky + 2].
struct SplatFoot {
    float wx[5], wy[5];
    uint32_t mx, my;
};
VK_HD void splat_axis(const SplatFilter &P, uint32_t i, float f, uint32_t extent, float w[5], uint32_t &mask) {
    const float c = f - 0.5f;
    mask = 0u;
#if defined(__HIPCC__) || defined(__HIP__)
#pragma unroll
#endif
    for (int k = -2; k <= 2; k++) {
        const float d = c - (float)k;
        const long long t = (long long)i + k;
        const bool in = d >= -P.radius && d < P.radius && t >= 0 && t < (long long)extent;
        w[k + 2] = in ? splat_w1(P, fabsf(d)) : 0.0f;
        if (in) mask |= 1u << (k + 2);
    }
}
// returns the contributions: the (pixel, sample) pairs in support and inside the frame
VK_HD uint32_t splat_weights(const SplatFilter &P, uint32_t ix, float fx, uint32_t iy, float fy, uint32_t width, uint32_t height,
                             SplatFoot &F) {
    splat_axis(P, ix, fx, width, F.wx, F.mx);
    splat_axis(P, iy, fy, height, F.wy, F.my);
    return (uint32_t)__builtin_popcount(F.mx) * (uint32_t)__builtin_popcount(F.my);
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// splat_deposit_kernel<TILED>: one lane per started id of a finished batch
struct SplatDepositArgs {
    const uint4 *result_state;     // vk_path_state[n]
    const uint32_t *result_status; // [n]
    const float2 *positions;       // [n] frame coordinates, or null: the state's pixel and the sample's own jitter
    unsigned long long *sums;      // [width * height * 4]: r, g, b, weight per pixel
    unsigned long long *counters;  // [SPLAT_STRIPES][SPLAT_STRIPE_WORDS]: deposited, dropped, clamped, skipped, contributions in each
    SplatFilter P;
    uint32_t n, width, height;
    float accum_clamp;             // accum_clamp_for(samples_per_pixel * ceil(2 radius)^2)
};
// splat_resolve_kernel: one lane per pixel
struct SplatResolveArgs {
    const long long *sums;
    float *out;                    // [width * height * 3]
    uint32_t n_pixels;
};

void launch_splat_deposit(const SplatDepositArgs &A, bool tiled);
void launch_splat_resolve(const SplatResolveArgs &A);
#endif

#endif
