// vk_tone.h — the kernels of vk_tone.hip as vk_api.hip sees them: their argument records and one thin launcher each (null stream,
// current device; the caller checks hipGetLastError).  The per-pixel code — luminance, the histogram's classification, the curves, the
// three transfers — is host-and-device: tests/emu/emu_tone.cpp builds it with g++.  The definition is include/vecchio_amd.h's ("display
// transform"); everything here is integers and unfused f32 and built without contraction.
#ifndef VK_TONE_H
#define VK_TONE_H

#include <stdint.h>

#include "vk_math.h"        // VK_HD, f32_bits, sat_u32, rng_for_stream, gen_f32

enum : uint32_t { TONE_CLAMP = 0u, TONE_REINHARD = 1u, TONE_HABLE = 2u, TONE_ACES = 3u };                 // = VK_TONE_*
enum : uint32_t { TONE_TRANSFER_REFERENCE = 0u, TONE_TRANSFER_SRGB = 1u, TONE_TRANSFER_GAMMA22 = 2u };   // = VK_TONE_TRANSFER_*
enum : uint32_t { TONE_FORM_LDS = 0u, TONE_FORM_PLAIN = 1u };                                            // = VK_TONE_FORM_*
enum : uint32_t { TONE_BINNED = 0u, TONE_BELOW = 1u, TONE_ABOVE = 2u, TONE_NONFINITE = 3u };             // the four counters, in order
constexpr uint32_t TONE_BINS = 640u, TONE_COUNTERS = 4u, TONE_TABLE = 510u;
constexpr uint64_t TONE_MAX_PIXELS = 1ull << 27;
constexpr float TONE_Y_MIN = 9.5367431640625e-07f, TONE_Y_MAX = 1048576.0f;      // 2^-20, 2^20
constexpr uint32_t TONE_BIN_BASE = (127u - 20u) << 4;                             // f32_bits(2^-20f) >> 19

VK_HD float tone_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

VK_HD bool tone_finite(float x) { return (vk::f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

// Where a pixel counts: TONE_BINS + TONE_NONFINITE / TONE_BELOW / TONE_ABOVE for the three counters, else its bin (< TONE_BINS).  A
// luminance that is no number cannot come of finite components; it would count below (the comparison is written so that it cannot index).
VK_HD uint32_t tone_classify(float r, float g, float b) {
    if (!(tone_finite(r) && tone_finite(g) && tone_finite(b))) return TONE_BINS + TONE_NONFINITE;
    const float Y = tone_luminance(r, g, b);
    if (!(Y >= TONE_Y_MIN)) return TONE_BINS + TONE_BELOW;
    if (Y >= TONE_Y_MAX) return TONE_BINS + TONE_ABOVE;
    return (vk::f32_bits(Y) >> 19) - TONE_BIN_BASE;
}

// ---- the curves: x = rgb * E in, y out.  p is the curve's parameter as the host computed it: REINHARD white * white, HABLE h(white).
VK_HD float tone_sanitise(float x) { return x > 0.0f ? (x < 1048576.0f ? x : 1048576.0f) : 0.0f; }

VK_HD float tone_hable(float v) {
    const float A = 0.15f, B = 0.5f, C = 0.1f, D = 0.2f, E_ = 0.02f, F = 0.3f;
    return ((v * (A * v + C * B) + D * E_) / (v * (A * v + B) + D * F)) - E_ / F;
}

template <uint32_t CURVE>
VK_HD void tone_curve(const float x[3], float p, float y[3]) {
    if (CURVE == TONE_CLAMP) {
        y[0] = x[0]; y[1] = x[1]; y[2] = x[2];
        return;
    }
    const float s[3] = {tone_sanitise(x[0]), tone_sanitise(x[1]), tone_sanitise(x[2])};
    if (CURVE == TONE_REINHARD) {
        const float Ys = tone_luminance(s[0], s[1], s[2]);
        const float k = (1.0f + Ys / p) / (1.0f + Ys);
        y[0] = s[0] * k; y[1] = s[1] * k; y[2] = s[2] * k;
    } else if (CURVE == TONE_HABLE) {
        y[0] = tone_hable(2.0f * s[0]) / p; y[1] = tone_hable(2.0f * s[1]) / p; y[2] = tone_hable(2.0f * s[2]) / p;
    } else {
        for (int c = 0; c < 3; c++) y[c] = (s[c] * (2.51f * s[c] + 0.03f)) / (s[c] * (2.43f * s[c] + 0.59f) + 0.14f);
    }
}

// ---- the transfers
// Vec3::to_color for one component, as vk_kernels.h to_color_u8 has it: sqrt, the hand-written clamp NaN falls through, * 256, `as u32`
VK_HD uint32_t tone_code_reference(float y) {
    const float v = sqrtf(y);
    const float cl = v < 0.0f ? 0.0f : (v > 0.999f ? 0.999f : v);
    return vk::sat_u32(256.0f * cl) & 255u;
}

// h[j - 1] = H[j], j = 1 .. 510.  The number of k in 1 .. 255 with y >= H[2k - ODD]: eight steps, no branch; a NaN counts none.
template <int ODD>
VK_HD uint32_t tone_count(const float *h, float y) {
    uint32_t pos = 0u;
    for (uint32_t step = 128u; step != 0u; step >>= 1) pos += y >= h[2u * (pos + step) - 1u - (uint32_t)ODD] ? step : 0u;
    return pos;
}

VK_HD uint32_t tone_code_table(const float *h, float y) { return tone_count<1>(h, y); }

VK_HD uint32_t tone_code_dither(const float *h, float y, float u) {
    const uint32_t base = tone_count<0>(h, y);
    const uint32_t at = base < 255u ? base : 254u;          // (255 stays 255: its interval is read nowhere)
    const float lo = at ? h[2u * at - 1u] : 0.0f, hi = h[2u * at + 1u];
    const float fr = (y - lo) / (hi - lo);
    return base < 255u ? base + (u < fr ? 1u : 0u) : 255u;
}

// One pixel: rgb the three input components, pixel its input index (y up), out its three codes
template <uint32_t CURVE, bool TABLE, bool DITHER>
VK_HD void tone_pixel(const float rgb[3], const float *h, float E, float p, uint64_t seed, uint32_t pixel, uint32_t out[3]) {
    const float x[3] = {rgb[0] * E, rgb[1] * E, rgb[2] * E};
    float y[3];
    tone_curve<CURVE>(x, p, y);
    if (!TABLE) {
        for (int c = 0; c < 3; c++) out[c] = tone_code_reference(y[c]);
    } else if (!DITHER) {
        for (int c = 0; c < 3; c++) out[c] = tone_code_table(h, y[c]);
    } else {
        vk::BuildRng g = vk::rng_for_stream(seed, (uint64_t)pixel);
        for (int c = 0; c < 3; c++) {
            const float u = vk::gen_f32(g);
            out[c] = tone_code_dither(h, y[c], u);
        }
    }
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// tone_meter_lds_kernel / tone_meter_plain_kernel
struct ToneMeterArgs {
    const float *rgb;              // [n_pixels * 3], 16-byte aligned
    uint32_t *bins;                // [TONE_BINS]
    unsigned long long *counters;  // [TONE_COUNTERS]
    uint32_t n_pixels;
};
// tone_encode_kernel<CURVE, TABLE, DITHER>
struct ToneEncodeArgs {
    const float *rgb;              // [width * height * 3], 16-byte aligned, y up
    const float *table;            // [TONE_TABLE] (table instances)
    uint8_t *out;                  // [width * height * 3], 4-byte aligned, row 0 the top
    uint32_t width, height;
    float E, p;
    uint64_t seed;
};

void launch_tone_meter(const ToneMeterArgs &A, uint32_t form);
void launch_tone_encode(const ToneEncodeArgs &A, uint32_t curve, bool table, bool dither);
#endif

#endif
