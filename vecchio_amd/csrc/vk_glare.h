// vk_glare.h — the kernels of vk_glare.hip as vk_api.hip sees them (their argument records, the launch plan and one thin launcher each:
// null stream, current device; the caller checks hipGetLastError) and the per-pixel code of the glare stage, host-and-device:
// tests/emu/emu_glare.cpp builds it with g++.  The definition is include/vecchio_amd.h's ("glare"); everything here is f32, unfused, in
// the order written there, and built without contraction.
//
// Every image is 3 floats a pixel, y up: the frame I, the planes B_1 .. B_{L-1} (the bright part, halved per level) and A_1 .. A_{L-2}
// (the weighted sums on their way up).  B_0 and A_0 are never stored.
#ifndef VK_GLARE_H
#define VK_GLARE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "vk_math.h"        // VK_HD, f32_bits

enum : uint32_t { GLARE_FORM_AUTO = 0u, GLARE_FORM_PLAIN = 1u, GLARE_FORM_FUSED = 2u };      // = VK_GLARE_FORM_*
constexpr uint32_t GLARE_MAX_LEVELS = 8u;
// The tail kernel's LDS, in floats of one colour component (a workgroup per component): every plane B_{t+1} .. B_7 side by side, and the
// two planes A alternates between on its way up.  64 512 bytes in all.
constexpr uint32_t GLARE_TAIL_B = 8192u, GLARE_TAIL_A = 6144u, GLARE_TAIL_A2 = 1792u;

VK_HD bool glare_finite(float x) { return (vk::f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

VK_HD int glare_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

VK_HD int glare_half(int n) { return (n + 1) >> 1; }

// the bright part B of one pixel I (threshold == 0: everything, sanitised as vk_tone does it)
VK_HD void glare_bright(const float I[3], float threshold, float B[3]) {
    if (!(glare_finite(I[0]) && glare_finite(I[1]) && glare_finite(I[2]))) {
        B[0] = 0.0f; B[1] = 0.0f; B[2] = 0.0f;
        return;
    }
    float s[3];
    for (int c = 0; c < 3; c++) s[c] = I[c] > 0.0f ? (I[c] < 1048576.0f ? I[c] : 1048576.0f) : 0.0f;
    if (threshold == 0.0f) {
        B[0] = s[0]; B[1] = s[1]; B[2] = s[2];
        return;
    }
    const float Y = (0.2126f * s[0] + 0.7152f * s[1]) + 0.0722f * s[2];
    const float f = fmaxf(0.0f, Y - threshold) / fmaxf(Y, 1e-20f);
    B[0] = s[0] * f; B[1] = s[1] * f; B[2] = s[2] * f;
}

// one output of the down filter from its four taps, and one of the up filter from its two
VK_HD float glare_down4(float a0, float a1, float a2, float a3) { return ((a0 + 3.0f * a1) + (3.0f * a2 + a3)) * 0.125f; }
VK_HD float glare_up2(float a, float nb) { return (3.0f * a + nb) * 0.25f; }

// the neighbour's index of the up filter: j - 1 for an even x, j + 1 for an odd one, clamped to the source
VK_HD int glare_up_nb(int x, int n) { return glare_clamp((x >> 1) + ((x & 1) ? 1 : -1), n); }

// One pixel of a down pass's source: the bright part of the frame (BRIGHT) or a stored plane
template <bool BRIGHT>
VK_HD void glare_source(const float *src, int sw, int x, int y, float threshold, float v[3]) {
    const size_t p = ((size_t)y * (size_t)sw + (size_t)x) * 3u;
    if (BRIGHT) {
        const float I[3] = {src[p], src[p + 1], src[p + 2]};
        glare_bright(I, threshold, v);
    } else {
        v[0] = src[p]; v[1] = src[p + 1]; v[2] = src[p + 2];
    }
}

// Down: pixel (X, Y) of the level above a sw x sh source: x first on the four source rows, then y
template <bool BRIGHT>
VK_HD void glare_down_pixel(const float *src, int sw, int sh, float threshold, int X, int Y, float out[3]) {
    float r[4][3];
    for (int k = 0; k < 4; k++) {
        const int y = glare_clamp(2 * Y - 1 + k, sh);
        float a[4][3];
        for (int j = 0; j < 4; j++) glare_source<BRIGHT>(src, sw, glare_clamp(2 * X - 1 + j, sw), y, threshold, a[j]);
        for (int c = 0; c < 3; c++) r[k][c] = glare_down4(a[0][c], a[1][c], a[2][c], a[3][c]);
    }
    for (int c = 0; c < 3; c++) out[c] = glare_down4(r[0][c], r[1][c], r[2][c], r[3][c]);
}

// Up: pixel (x, y) of the level below a sw x sh source whose values are scale * src (scale = 1 for a stored A, c_{L-1} for B_{L-1}): x
// first on the two source rows, then y
VK_HD void glare_up_pixel(const float *src, int sw, int sh, float scale, int x, int y, float out[3]) {
    const int jx = x >> 1, nx = glare_up_nb(x, sw), jy = y >> 1, ny = glare_up_nb(y, sh);
    const size_t pj = ((size_t)jy * (size_t)sw) * 3u, pn = ((size_t)ny * (size_t)sw) * 3u;
    for (int c = 0; c < 3; c++) {
        const float uj = glare_up2(scale * src[pj + (size_t)jx * 3u + c], scale * src[pj + (size_t)nx * 3u + c]);
        const float un = glare_up2(scale * src[pn + (size_t)jx * 3u + c], scale * src[pn + (size_t)nx * 3u + c]);
        out[c] = glare_up2(uj, un);
    }
}

// Composite: out = I + strength * (A_0 - B), A_0 = c0 * B + up (up: Up(A_1) at this pixel; has_up false for L = 1)
VK_HD void glare_composite_pixel(const float I[3], float threshold, float c0, float strength, bool has_up, const float up[3], float out[3]) {
    float B[3];
    glare_bright(I, threshold, B);
    for (int c = 0; c < 3; c++) {
        const float A0 = has_up ? c0 * B[c] + up[c] : c0 * B[c];
        out[c] = I[c] + strength * (A0 - B[c]);
    }
}

// the weights c_l = (float)(p_l / S), p_l = falloff^l, in f64 basic arithmetic
inline void glare_weights(uint32_t levels, float falloff, float c[GLARE_MAX_LEVELS]) {
    double p[GLARE_MAX_LEVELS], S = 0.0;
    for (uint32_t l = 0; l < GLARE_MAX_LEVELS; l++) { p[l] = l ? p[l - 1] * (double)falloff : 1.0; c[l] = 0.0f; }
    for (uint32_t l = 0; l < levels; l++) S += p[l];
    for (uint32_t l = 0; l < levels; l++) c[l] = (float)(p[l] / S);
}

// the sizes of the eight levels of a width x height frame
struct GlareDims { int w[GLARE_MAX_LEVELS], h[GLARE_MAX_LEVELS]; };
inline GlareDims glare_dims(uint32_t width, uint32_t height) {
    GlareDims d;
    d.w[0] = (int)width; d.h[0] = (int)height;
    for (uint32_t l = 1; l < GLARE_MAX_LEVELS; l++) { d.w[l] = glare_half(d.w[l - 1]); d.h[l] = glare_half(d.h[l - 1]); }
    return d;
}

// The first level t >= 1 from which the tail kernel can take over: B_{t+1} .. B_7 fit its B store side by side, B_{t+1}'s and B_{t+2}'s
// sizes the two A stores.  A function of the frame's size alone; 7 if none does (a tail then has nothing to do).
inline uint32_t glare_tail_level(const GlareDims &d) {
    for (uint32_t t = 1; t + 1 < GLARE_MAX_LEVELS; t++) {
        uint64_t sum = 0;
        for (uint32_t l = t + 1; l < GLARE_MAX_LEVELS; l++) sum += (uint64_t)d.w[l] * (uint64_t)d.h[l];
        const uint64_t n1 = (uint64_t)d.w[t + 1] * (uint64_t)d.h[t + 1];
        const uint64_t n2 = t + 2 < GLARE_MAX_LEVELS ? (uint64_t)d.w[t + 2] * (uint64_t)d.h[t + 2] : 0u;
        if (sum <= GLARE_TAIL_B && n1 <= GLARE_TAIL_A && n2 <= GLARE_TAIL_A2) return t;
    }
    return GLARE_MAX_LEVELS - 1u;
}

// The kernels one apply launches: PLAIN max(1, 2L - 2); FUSED fewer for L >= 3 (DESIGN.md "Glare")
inline uint32_t glare_launch_count(uint32_t width, uint32_t height, uint32_t L, uint32_t form) {
    if (L <= 1u) return 1u;
    if (form == GLARE_FORM_PLAIN) return 2u * L - 2u;
    const uint32_t t = glare_tail_level(glare_dims(width, height));
    const bool tail = t + 2u <= L;
    const uint32_t m = tail ? t : L - 1u;                    // B_1 .. B_m go to global memory
    const uint32_t downs = m >= 2u ? m - 1u : m;             // the first launch makes two levels
    const uint32_t ups = (tail ? t : L - 1u) - 1u;           // A_{top - 1} .. A_1
    return downs + (tail ? 1u : 0u) + ups + 1u;
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// glare_down_kernel<BRIGHT, LDS>: dst (level l + 1) from src (level l: the frame when BRIGHT)
struct GlareDownArgs {
    const float *src;
    float *dst;
    uint32_t sw, sh;               // the source's size; dst is ceil(sw / 2) x ceil(sh / 2)
    float threshold;
};
// glare_down2_kernel: B_1 and B_2 from the frame in one launch
struct GlareDown2Args {
    const float *src;
    float *b1, *b2;
    uint32_t sw, sh;
    float threshold;
};
// glare_up_kernel: dst (level l) = c * b + Up(scale * src (level l + 1))
struct GlareUpArgs {
    const float *src, *b;
    float *dst;
    uint32_t w, h;                 // dst's and b's size; src is ceil(w / 2) x ceil(h / 2)
    float c, scale;
};
// glare_composite_kernel: out = I + strength * ((c0 * B + Up(scale * src)) - B); src null for L = 1
struct GlareCompositeArgs {
    const float *in, *src;
    float *out;
    uint32_t w, h;
    float c0, scale, strength, threshold;
};
// glare_tail_kernel: A_t from B_t, levels t .. L - 1 in LDS, a workgroup per colour component
struct GlareTailArgs {
    const float *bt;
    float *at;
    uint32_t w, h;                 // level t's size
    uint32_t t, levels;
    float c[GLARE_MAX_LEVELS];
};

void launch_glare_down(const GlareDownArgs &A, bool bright, bool lds);
void launch_glare_down2(const GlareDown2Args &A);
void launch_glare_up(const GlareUpArgs &A);
void launch_glare_composite(const GlareCompositeArgs &A);
void launch_glare_tail(const GlareTailArgs &A);
#endif

#endif
