// vk_upsample.h — the kernels of vk_upsample.hip as vk_api.hip sees them (their argument records and one thin launcher each: null stream,
// current device; the caller checks hipGetLastError) and the per-pixel code of guided upsampling, host-and-device:
// tests/emu/emu_upsample.cpp builds it with g++.  The definition is include/vecchio_amd.h's ("guided upsampling"); everything here is
// f32, unfused, in the order written there, and built without contraction.
//
// A low pixel q is three 16-byte records, one per plane:
//   P0[q] = (I_r, I_g, I_b, valid)     demodulated colour; valid 1 or 0 (an INVALID pixel's I and V are 0)
//   P1[q] = (V_r, V_g, V_b, z)         variance of the demodulated colour; depth, +inf = nothing hit (or no depth loaded)
//   P2[q] = (n^x, n^y, n^z, has)       unit normal and has 1, or (0, 0, 0, 0) = NO NORMAL (or no normal loaded)
#ifndef VK_UPSAMPLE_H
#define VK_UPSAMPLE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "vk_math.h"        // VK_HD, f32_bits

enum : uint32_t { UPSAMPLE_FORM_AUTO = 0u, UPSAMPLE_FORM_PLAIN = 1u, UPSAMPLE_FORM_TILED = 2u };      // = VK_UPSAMPLE_FORM_*
enum : uint32_t { UP_NORMAL = 1u, UP_DEPTH = 2u };          // UpsampleArgs::flags: the terms that are on (a guide on both sides)
// the tiled form: a workgroup's tile of high pixels and the low footprint it stages.  The mapping's ratio is <= 1, so UP_TX high pixels
// span at most UP_TX low ones, and the 4 x 4 taps add one in front and two behind.
constexpr int UP_TX = 32, UP_TY = 8, UP_FW = UP_TX + 4, UP_FH = UP_TY + 4;

struct alignas(16) UpRec { float x, y, z, w; };

VK_HD bool up_finite(float x) { return (vk::f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

// E(x) = max(0, 1 - x/8)^8 (vk_denoise's); fmaxf drops a NaN, so E(NaN) = 0
VK_HD float up_falloff(float x) {
    float t = fmaxf(0.0f, 1.0f - x * 0.125f);
    t = t * t; t = t * t;
    return t * t;
}

// a high pixel's centre in low pixels, along one axis
VK_HD float up_map(int X, float r) { return ((float)X + 0.5f) * r - 0.5f; }

// The depth slope along one axis from the two one-sided differences dl = z - z_left and dr = z_right - z (has_l, has_r: the neighbour is
// in the image and finite): with both, the one smaller in magnitude where they agree in sign and 0 where they do not (minmod: a central
// difference would take a depth edge next to the pixel for a slope and let the far side in); with one, that one; with none, 0.
VK_HD float up_slope(bool has_l, float dl, bool has_r, float dr) {
    if (has_l && has_r) return dl * dr > 0.0f ? (dl > 0.0f ? fminf(dl, dr) : fmaxf(dl, dr)) : 0.0f;
    return has_r ? dr : (has_l ? dl : 0.0f);
}

// the unit normal of n (false, and (0, 0, 0): NO NORMAL)
VK_HD bool up_normal(float n0, float n1, float n2, float out[3]) {
    const float l2 = (n0 * n0 + n1 * n1) + n2 * n2;
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    if (l2 < 1e-12f || !up_finite(l2)) return false;
    const float l = sqrtf(l2);
    out[0] = n0 / l; out[1] = n1 / l; out[2] = n2 / l;
    return true;
}

// Prepare: the three records of low pixel q from the loaded images (stderr3, albedo, normal, depth may be null)
VK_HD void upsample_prepare_pixel(const float *color, const float *stderr3, const float *albedo, const float *normal, const float *depth,
                                  float albedo_floor, size_t q, UpRec &p0, UpRec &p1, UpRec &p2) {
    const float c0 = color[q * 3], c1 = color[q * 3 + 1], c2 = color[q * 3 + 2];
    bool valid = up_finite(c0) && up_finite(c1) && up_finite(c2);
    float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
    if (albedo) {
        a0 = fmaxf(albedo[q * 3], albedo_floor); a1 = fmaxf(albedo[q * 3 + 1], albedo_floor); a2 = fmaxf(albedo[q * 3 + 2], albedo_floor);
    }
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (stderr3) {
        const float e0 = stderr3[q * 3], e1 = stderr3[q * 3 + 1], e2 = stderr3[q * 3 + 2];
        valid = valid && up_finite(e0) && up_finite(e1) && up_finite(e2);
        const float s0 = e0 / a0, s1 = e1 / a1, s2 = e2 / a2;
        v0 = s0 * s0; v1 = s1 * s1; v2 = s2 * s2;
    }
    float z = INFINITY;
    if (depth) { const float d = depth[q]; z = up_finite(d) ? d : INFINITY; }
    if (valid) { p0.x = c0 / a0; p0.y = c1 / a1; p0.z = c2 / a2; p0.w = 1.0f; p1.x = v0; p1.y = v1; p1.z = v2; }
    else { p0.x = 0.0f; p0.y = 0.0f; p0.z = 0.0f; p0.w = 0.0f; p1.x = 0.0f; p1.y = 0.0f; p1.z = 0.0f; }
    p1.w = z;
    float n[3] = {0.0f, 0.0f, 0.0f};
    bool has = false;
    if (normal) has = up_normal(normal[q * 3], normal[q * 3 + 1], normal[q * 3 + 2], n);
    p2.x = n[0]; p2.y = n[1]; p2.z = n[2]; p2.w = has ? 1.0f : 0.0f;
}

// what one apply reads and writes (the kernels' argument record, and the host build's)
struct UpsampleArgs {
    const UpRec *P0, *P1, *P2;                     // the prepared low planes, [w * h] each
    const float *albedo_hi, *normal_hi, *depth_hi; // [W * H * 3], [W * H * 3], [W * H]; null = not given
    float *out, *stderr3_out;                      // [W * H * 3]; stderr3_out may be null
    uint32_t *counts;                              // [2]: fallback_pixels, empty_pixels (zeroed by the caller)
    uint32_t w, h, W, H;
    float rx, ry, sx, sy;                          // (float)((double)(w - 1) / (double)(W - 1)) .., (float)((double)(W - 1) / (double)(w - 1)) ..
    float sigma_z, albedo_floor;
    uint32_t normal_squarings, flags;              // UP_NORMAL | UP_DEPTH
};

// the two ratios of one axis: lo and hi are both >= 2
inline void upsample_ratios(uint32_t lo, uint32_t hi, float &r, float &s) {
    r = (float)((double)(lo - 1u) / (double)(hi - 1u));
    s = (float)((double)(hi - 1u) / (double)(lo - 1u));
}

// One high pixel (X, Y), every form: fetch(tx, ty, p0, p1, p2) reads the records of the in-image low pixel (tx, ty).  Writes out (and
// stderr3_out) and returns 0 = filtered, 1 = fell back to the tent alone, 2 = no valid tap (out = 0; counts as a fallback too).
// The guided sums and the tent-alone sums are taken in one sweep: each in tap order from 0, as the definition has them.
template <class Fetch>
VK_HD int upsample_pixel(const UpsampleArgs &A, int X, int Y, Fetch fetch) {
    const int w = (int)A.w, h = (int)A.h, W = (int)A.W, H = (int)A.H;
    const size_t P = (size_t)Y * (size_t)W + (size_t)X;
    const float px = up_map(X, A.rx), py = up_map(Y, A.ry);
    const int x0 = (int)floorf(px), y0 = (int)floorf(py);
    float nP[3] = {0.0f, 0.0f, 0.0f};
    bool p_has = false;
    if (A.flags & UP_NORMAL) p_has = up_normal(A.normal_hi[P * 3], A.normal_hi[P * 3 + 1], A.normal_hi[P * 3 + 2], nP);
    float zP = INFINITY, gx = 0.0f, gy = 0.0f;
    if (A.flags & UP_DEPTH) {
        const float z = A.depth_hi[P];
        if (up_finite(z)) {
            zP = z;
            const float zl = X > 0 ? A.depth_hi[P - 1] : INFINITY, zr = X + 1 < W ? A.depth_hi[P + 1] : INFINITY;
            const float zd = Y > 0 ? A.depth_hi[P - (size_t)W] : INFINITY, zu = Y + 1 < H ? A.depth_hi[P + (size_t)W] : INFINITY;
            const bool l = up_finite(zl), r = up_finite(zr), d = up_finite(zd), u = up_finite(zu);
            gx = up_slope(l, z - zl, r, zr - z);
            gy = up_slope(d, z - zd, u, zu - z);
        }
    }
    const bool p_far = zP == INFINITY;
    float Wg = 0.0f, Jg[3] = {0.0f, 0.0f, 0.0f}, Ug[3] = {0.0f, 0.0f, 0.0f};       // guided
    float Wf = 0.0f, Jf[3] = {0.0f, 0.0f, 0.0f}, Uf[3] = {0.0f, 0.0f, 0.0f};       // the tent alone
    for (int ty = y0 - 1; ty <= y0 + 2; ty++) {
        if (ty < 0 || ty >= h) continue;
        const float ky = fmaxf(0.0f, 1.0f - fabsf(py - (float)ty) * 0.5f);
        for (int tx = x0 - 1; tx <= x0 + 2; tx++) {
            if (tx < 0 || tx >= w) continue;
            UpRec q0, q1, q2;
            fetch(tx, ty, q0, q1, q2);
            if (q0.w == 0.0f) continue;                  // INVALID
            const float kx = fmaxf(0.0f, 1.0f - fabsf(px - (float)tx) * 0.5f);
            const float k = kx * ky;
            Wf += k;
            Jf[0] += k * q0.x; Jf[1] += k * q0.y; Jf[2] += k * q0.z;
            Uf[0] += (k * k) * q1.x; Uf[1] += (k * k) * q1.y; Uf[2] += (k * k) * q1.z;
            float wn = 1.0f, xz = 0.0f;
            if (A.flags & UP_NORMAL) {
                const bool q_has = q2.w != 0.0f;
                if (p_has != q_has) wn = 0.0f;
                else if (p_has) {
                    wn = fmaxf(0.0f, (nP[0] * q2.x + nP[1] * q2.y) + nP[2] * q2.z);
                    for (uint32_t i = 0; i < A.normal_squarings; i++) wn = wn * wn;
                }
            }
            if (A.flags & UP_DEPTH) {
                const bool q_far = q1.w == INFINITY;
                if (p_far != q_far) continue;
                if (!p_far) {
                    const float ux = ((float)tx - px) * A.sx, uy = ((float)ty - py) * A.sy;
                    xz = fabsf(zP - q1.w) / (A.sigma_z * (fabsf(gx * ux + gy * uy) + 0.001f * zP));
                }
            }
            const float wt = (k * wn) * up_falloff(xz);
            Wg += wt;
            Jg[0] += wt * q0.x; Jg[1] += wt * q0.y; Jg[2] += wt * q0.z;
            Ug[0] += (wt * wt) * q1.x; Ug[1] += (wt * wt) * q1.y; Ug[2] += (wt * wt) * q1.z;
        }
    }
    int what = 0;
    if (Wg < 1e-4f) {
        what = 1;
        Wg = Wf;
        for (int c = 0; c < 3; c++) { Jg[c] = Jf[c]; Ug[c] = Uf[c]; }
    }
    if (Wg < 1e-4f) {
        what = 2;
        for (int c = 0; c < 3; c++) {
            A.out[P * 3 + c] = 0.0f;
            if (A.stderr3_out) A.stderr3_out[P * 3 + c] = 0.0f;
        }
        return what;
    }
    for (int c = 0; c < 3; c++) {
        const float a = A.albedo_hi ? fmaxf(A.albedo_hi[P * 3 + c], A.albedo_floor) : 1.0f;
        A.out[P * 3 + c] = (Jg[c] / Wg) * a;
        if (A.stderr3_out) A.stderr3_out[P * 3 + c] = (sqrtf(Ug[c]) / Wg) * a;
    }
    return what;
}

// AUTO's rule, a function of the sizes alone: the form that was measured faster on the MI355X (tools/upsample_report.py, DESIGN.md
// "Guided upsampling").  At 1920 x 1080, 900 x 900 and 800 x 800, from half and from quarter size, the tiled form took 0.80 to 0.95 times
// the plain form's time per call in a stream of calls, in every one of the six cells; nothing smaller was measured, and nothing there
// speaks for the plain form, so AUTO is the tiled form at every size.
inline uint32_t upsample_auto_form(uint32_t w, uint32_t h, uint32_t W, uint32_t H) {
    (void)w; (void)h; (void)W; (void)H;
    return UPSAMPLE_FORM_TILED;
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// upsample_prepare_kernel: the three planes from the handle's copy of the loaded images
struct UpsamplePrepareArgs {
    const float *color, *stderr3, *albedo, *normal, *depth;        // all but color may be null
    UpRec *P0, *P1, *P2;
    uint32_t w, h;
    float albedo_floor;
};

void launch_upsample_prepare(const UpsamplePrepareArgs &A);
void launch_upsample_apply(const UpsampleArgs &A, uint32_t form);      // UPSAMPLE_FORM_PLAIN or _TILED
#endif

#endif
