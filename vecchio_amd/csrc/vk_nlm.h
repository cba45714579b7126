// vk_nlm.h — the kernels of vk_nlm.hip as vk_api.hip sees them (their argument records and one thin launcher each: null stream, current
// device; the caller checks hipGetLastError) and the per-pixel code of the non-local-means filter, host-and-device:
// tests/emu/emu_nlm.cpp builds it with g++.  The definition is include/vecchio_amd.h's ("non-local means"); everything here is f32,
// unfused, in the order written there, and built without contraction.
//
// The planes a handle owns, component-major (plane c of n = width * height floats at base + c * n: a wave reads consecutive dwords):
//   I  [3][n]   demodulated colour; an INVALID pixel's raw colour
//   V  [3][n]   variance per component; an INVALID pixel's raw stderr3
//   Vf [3][n]   V through k3 over the adjacent valid pixels; Vf[0][p] = -1 marks an INVALID pixel (Vf is >= 0 otherwise: V is a square)
//   a  [3][n]   the albedo the pixel was divided by (1 without albedo)
#ifndef VK_NLM_H
#define VK_NLM_H

#include <math.h>
#include <stdint.h>

#include "vk_math.h"        // VK_HD, f32_bits

enum : uint32_t { NLM_FORM_AUTO = 0u, NLM_FORM_PLAIN = 1u, NLM_FORM_TILED = 2u };      // = VK_NLM_FORM_*
constexpr uint32_t NLM_MAX_R = 10u, NLM_MAX_F = 3u;

struct NlmPlanes {
    const float *I, *V, *Vf, *a;
    uint32_t width, height;
};

VK_HD bool nlm_finite(float x) { return (vk::f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

// E(x) = max(0, 1 - x/8)^8, vk_denoise's: fmaxf drops a NaN
VK_HD float nlm_falloff(float x) {
    float t = fmaxf(0.0f, 1.0f - x * 0.125f);
    t = t * t; t = t * t;
    return t * t;
}

// Prepare's first half for one pixel: a, I = color / a and V = (stderr / a)^2 per component; false = INVALID (I and V then hold the raw
// colour and stderr3).  albedo may be null.
VK_HD bool nlm_demodulate(const float *color, const float *stderr3, const float *albedo, float albedo_floor, size_t p, float I[3], float V[3],
                          float a[3]) {
    bool valid = true;
    for (int c = 0; c < 3; c++) {
        const float col = color[p * 3 + c], se = stderr3[p * 3 + c];
        valid = valid && nlm_finite(col) && nlm_finite(se);
        a[c] = albedo ? fmaxf(albedo[p * 3 + c], albedo_floor) : 1.0f;
        I[c] = col / a[c];
        const float s = se / a[c];
        V[c] = s * s;
    }
    if (!valid)
        for (int c = 0; c < 3; c++) { I[c] = color[p * 3 + c]; V[c] = stderr3[p * 3 + c]; }
    return valid;
}

// Prepare for the pixel (x, y): its four plane entries.  Vf is vk_denoise's Vg recipe per component (rows bottom to top, x ascending,
// k3 = (1 2 1; 2 4 2; 1 2 1), both sums from 0), over V as nlm_demodulate gives it for each neighbour.
VK_HD void nlm_prepare_pixel(const float *color, const float *stderr3, const float *albedo, float albedo_floor, int w, int h, int x, int y,
                             float I[3], float V[3], float Vf[3], float a[3]) {
    const size_t p = (size_t)y * (size_t)w + (size_t)x;
    if (!nlm_demodulate(color, stderr3, albedo, albedo_floor, p, I, V, a)) {
        Vf[0] = -1.0f; Vf[1] = 0.0f; Vf[2] = 0.0f;
        return;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f}, ws = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            float Iq[3], Vq[3], aq[3];
            if (!nlm_demodulate(color, stderr3, albedo, albedo_floor, (size_t)qy * (size_t)w + (size_t)qx, Iq, Vq, aq)) continue;
            const float kw = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
            for (int c = 0; c < 3; c++) acc[c] += kw * Vq[c];
            ws += kw;
        }
    for (int c = 0; c < 3; c++) Vf[c] = acc[c] / ws;
}

// One channel of the pair term: num / den
VK_HD float nlm_pair_channel(float Ia, float Ib, float Vfa, float Vfb, float alpha, float kk) {
    const float d = Ia - Ib;
    const float num = d * d - alpha * (Vfa + fminf(Vfa, Vfb));
    const float den = 1e-10f + kk * (Vfa + Vfb);
    return num / den;
}

// e(a, b) for two valid pixels; kk = k * k
VK_HD float nlm_pair(const float Ia[3], const float Vfa[3], const float Ib[3], const float Vfb[3], float alpha, float kk) {
    return (nlm_pair_channel(Ia[0], Ib[0], Vfa[0], Vfb[0], alpha, kk) + nlm_pair_channel(Ia[1], Ib[1], Vfa[1], Vfb[1], alpha, kk)) +
           nlm_pair_channel(Ia[2], Ib[2], Vfa[2], Vfb[2], alpha, kk);
}

// the weight of an offset from its patch sum S over n >= 1 pairs
VK_HD float nlm_weight(float S, uint32_t n) {
    const float D = S / (float)(3u * n);
    return D != D ? 0.0f : nlm_falloff(fmaxf(0.0f, D));
}

// the accumulators of one pixel, in offset order
struct NlmSums {
    float W, J[3], U[3];
};

VK_HD void nlm_sums_clear(NlmSums &s) {
    s.W = 0.0f;
    for (int c = 0; c < 3; c++) { s.J[c] = 0.0f; s.U[c] = 0.0f; }
}

VK_HD void nlm_sums_add(NlmSums &s, float w, const float Iq[3], const float Vq[3]) {
    s.W += w;
    for (int c = 0; c < 3; c++) { s.J[c] += w * Iq[c]; s.U[c] += (w * w) * Vq[c]; }
}

VK_HD void nlm_finish(const NlmSums &s, const float a[3], float out[3], float se[3]) {
    for (int c = 0; c < 3; c++) {
        out[c] = (s.J[c] / s.W) * a[c];
        se[c] = (sqrtf(s.U[c]) / s.W) * a[c];
    }
}

VK_HD bool nlm_valid_at(const NlmPlanes &P, int x, int y) {
    if (x < 0 || y < 0 || x >= (int)P.width || y >= (int)P.height) return false;
    return !(P.Vf[(size_t)y * P.width + (size_t)x] < 0.0f);
}

// The definition for the pixel (x, y), evaluated directly from the planes: what the PLAIN form and the host build run.
VK_HD void nlm_filter_pixel(const NlmPlanes &P, int x, int y, int R, int F, float alpha, float kk, float out[3], float se[3]) {
    const size_t n = (size_t)P.width * P.height, p = (size_t)y * P.width + (size_t)x;
    if (P.Vf[p] < 0.0f) {                // invalid: out is its colour, stderr3_out its stderr3
        for (int c = 0; c < 3; c++) { out[c] = P.I[c * n + p]; se[c] = P.V[c * n + p]; }
        return;
    }
    NlmSums s;
    nlm_sums_clear(s);
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++) {
            const int qx = x + ox, qy = y + oy;
            if (!nlm_valid_at(P, qx, qy)) continue;
            const size_t q = (size_t)qy * P.width + (size_t)qx;
            float w = 1.0f;
            if (ox != 0 || oy != 0) {
                float S = 0.0f;
                uint32_t cnt = 0u;
                for (int j = -F; j <= F; j++) {
                    float r = 0.0f;
                    uint32_t m = 0u;
                    for (int i = -F; i <= F; i++) {
                        const int ax = x + i, ay = y + j, bx = qx + i, by = qy + j;
                        float e = 0.0f;
                        if (nlm_valid_at(P, ax, ay) && nlm_valid_at(P, bx, by)) {
                            const size_t ia = (size_t)ay * P.width + (size_t)ax, ib = (size_t)by * P.width + (size_t)bx;
                            const float Ia[3] = {P.I[ia], P.I[n + ia], P.I[2 * n + ia]}, Ib[3] = {P.I[ib], P.I[n + ib], P.I[2 * n + ib]};
                            const float Va[3] = {P.Vf[ia], P.Vf[n + ia], P.Vf[2 * n + ia]}, Vb[3] = {P.Vf[ib], P.Vf[n + ib], P.Vf[2 * n + ib]};
                            e = nlm_pair(Ia, Va, Ib, Vb, alpha, kk);
                            m += 1u;
                        }
                        r += e;
                    }
                    S += r; cnt += m;
                }
                w = nlm_weight(S, cnt);
            }
            const float Iq[3] = {P.I[q], P.I[n + q], P.I[2 * n + q]}, Vq[3] = {P.V[q], P.V[n + q], P.V[2 * n + q]};
            nlm_sums_add(s, w, Iq, Vq);
        }
    const float a[3] = {P.a[p], P.a[n + p], P.a[2 * n + p]};
    nlm_finish(s, a, out, se);
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// nlm_prepare_kernel
struct NlmPrepareArgs {
    const float *color, *stderr3, *albedo;      // [n * 3] each; albedo may be null
    float *I, *V, *Vf, *a;                      // the handle's planes, [3][n] each
    uint32_t width, height;
    float albedo_floor;
};
// nlm_filter_kernel<FORM, HALO>
struct NlmFilterArgs {
    NlmPlanes P;
    float *out, *stderr3_out;                   // [n * 3]; stderr3_out may be null
    int R, F;
    float alpha, kk;
};

constexpr int NLM_TILED_SMALL_HALO = 6, NLM_TILED_LARGE_HALO = 13;      // the two instances of the tiled form: R + F up to these

void launch_nlm_prepare(const NlmPrepareArgs &A);
void launch_nlm_filter(const NlmFilterArgs &A, uint32_t form);          // form: NLM_FORM_PLAIN or NLM_FORM_TILED
#endif

#endif
