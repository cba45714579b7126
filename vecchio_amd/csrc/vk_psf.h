// vk_psf.h — the kernels of vk_psf.hip as vk_api.hip sees them (their argument records and one thin launcher each: null stream, current
// device; the caller checks hipGetLastError) and the per-element code of the point-spread stage, host-and-device: tests/emu/emu_psf.cpp
// builds it with g++.  The definition is include/vecchio_amd.h's ("point-spread function"); everything on the device is f32, unfused,
// in the order written there, and built without contraction.  The tables and the kernel's normalisation are f64 on the host.
//
// A plane is Px x Py complex values (PsfC, 8 bytes), row y at y * Px; a handle has three for the frame's transform F and three for the
// loaded kernel's G, one per colour component.
#ifndef VK_PSF_H
#define VK_PSF_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "vk_math.h"        // VK_HD, f32_bits

enum : uint32_t { PSF_FORM_AUTO = 0u, PSF_FORM_PLAIN = 1u, PSF_FORM_LDS = 2u };      // = VK_PSF_FORM_*
constexpr uint32_t PSF_MIN_K = 3u, PSF_MAX_K = 1023u, PSF_MAX_N = 4096u;
// the line kernel's LDS in complex values: one row of up to 4096 (or several shorter rows); a tile of adjacent columns of up to 8192
constexpr uint32_t PSF_ROW_CAP = 4096u, PSF_COL_CAP = 8192u, PSF_ROW_MAX_LINES = 16u, PSF_COL_MAX_LINES = 32u;

struct PsfC { float re, im; };

VK_HD bool psf_finite(float x) { return (vk::f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

// the smallest power of two >= n (n >= 1) and its exponent
VK_HD uint32_t psf_pow2(uint32_t n) { uint32_t p = 1u; while (p < n) p <<= 1; return p; }
VK_HD uint32_t psf_log2(uint32_t p) { uint32_t m = 0u; while ((1u << m) < p) m++; return m; }

// the m-bit reversal of i
VK_HD uint32_t psf_rev(uint32_t i, uint32_t m) {
    uint32_t r = 0u;
    for (uint32_t b = 0; b < m; b++) r |= ((i >> b) & 1u) << (m - 1u - b);
    return r;
}

// t = v * w, the one multiply of the stage: the butterfly's and the product's
VK_HD PsfC psf_mul(PsfC v, PsfC w) {
    PsfC t;
    t.re = v.re * w.re - v.im * w.im;
    t.im = v.re * w.im + v.im * w.re;
    return t;
}

// one butterfly in place: (u, v) -> (u + v w, u - v w); the inverse transform's w has its imaginary part negated
VK_HD void psf_butterfly(PsfC &u, PsfC &v, PsfC w, bool inverse) {
    if (inverse) w.im = -w.im;
    const PsfC t = psf_mul(v, w);
    const PsfC a = {u.re + t.re, u.im + t.im}, b = {u.re - t.re, u.im - t.im};
    u = a; v = b;
}

// butterfly i (0 .. N/2 - 1) of stage s (1 .. m) of a length-2^m line: the index p of u (v is at p + half) and of w in the table
VK_HD void psf_butterfly_at(uint32_t i, uint32_t s, uint32_t m, uint32_t &p, uint32_t &half, uint32_t &wk) {
    half = 1u << (s - 1u);
    const uint32_t j = i & (half - 1u);
    p = ((i >> (s - 1u)) << s) + j;
    wk = j << (m - s);
}

// the bright part B of one pixel I: vk_glare's definition, verbatim
VK_HD void psf_bright(const float I[3], float threshold, float B[3]) {
    if (!(psf_finite(I[0]) && psf_finite(I[1]) && psf_finite(I[2]))) {
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

// one component of the composite: out = I + strength * (C - B), C = re * scale (scale = 1 / (Px Py), a power of two); a component that
// is not finite stays what it was
VK_HD float psf_composite(float I, float B, float re, float scale, float strength) {
    if (!psf_finite(I)) return I;
    const float C = re * scale;
    return I + strength * (C - B);
}

// where the kernel's tap (kx, ky) of a K x K kernel lands in the Px x Py plane: its centre at (0, 0), wrapped
VK_HD uint32_t psf_wrap(uint32_t k, uint32_t K, uint32_t P) {
    const uint32_t r = (K - 1u) / 2u;
    return k >= r ? k - r : P - (r - k);
}

// the value of the placed kernel at (x, y) of the plane: tap (x + r, y + r) for x, y in -r .. r (mod Px, Py), else +0
VK_HD float psf_placed(const float *kernel, uint32_t K, uint32_t c, uint32_t Px, uint32_t Py, uint32_t x, uint32_t y) {
    const uint32_t r = (K - 1u) / 2u;
    uint32_t kx, ky;
    if (x <= r) kx = x + r; else if (x >= Px - r) kx = x - (Px - r); else return 0.0f;
    if (y <= r) ky = y + r; else if (y >= Py - r) ky = y - (Py - r); else return 0.0f;
    return kernel[((size_t)ky * K + kx) * 3u + c];
}

// ---- the host's f64 parts -------------------------------------------------------------------------------------------------------------

// The twiddle table of a length N = 2^m (include/vecchio_amd.h "Twiddle tables"): N/2 entries (N = 1: none), f64 with + - * / and sqrt
// only.  R_q = (cos, sin)(pi / 2^q): R_1 = (0, 1); c_{q+1} = sqrt((1 + c_q) / 2), s_{q+1} = s_q / (2 c_{q+1}).  z_k = the product over
// the set bits t of k, ascending, of R_{m-1-t}, from z = (1, 0), each product (a.re b.re - a.im b.im, a.re b.im + a.im b.re).
// T[k] = ((float)z.re, (float)(0 - z.im)).
inline std::vector<PsfC> psf_twiddles(uint32_t N) {
    const uint32_t m = psf_log2(N);
    std::vector<PsfC> T(N / 2u);
    double c[16], s[16];
    c[1] = 0.0; s[1] = 1.0;
    for (uint32_t q = 1; q + 1u < 16u; q++) {
        c[q + 1] = sqrt((1.0 + c[q]) / 2.0);
        s[q + 1] = s[q] / (2.0 * c[q + 1]);
    }
    for (uint32_t k = 0; k < N / 2u; k++) {
        double zr = 1.0, zi = 0.0;
        for (uint32_t t = 0; t + 1u < m; t++) {
            if (!((k >> t) & 1u)) continue;
            const uint32_t q = m - 1u - t;
            const double nr = zr * c[q] - zi * s[q], ni = zr * s[q] + zi * c[q];
            zr = nr; zi = ni;
        }
        T[k].re = (float)zr; T[k].im = (float)(0.0 - zi);
    }
    return T;
}

// Why a kernel cannot be loaded, or null; then `out` (K * K * 3 floats) holds it normalised: k_c[i] = (float)(k_c[i] / S_c), S_c the f64
// sum of channel c in ascending index order
inline const char *psf_normalise(uint32_t K, const float *kernel, float *out) {
    const size_t n = (size_t)K * K;
    double S[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < n * 3u; i++) {
        if (!psf_finite(kernel[i])) return "kernel component not finite";
        if (kernel[i] < 0.0f) return "kernel component negative";
    }
    for (size_t i = 0; i < n; i++) for (int c = 0; c < 3; c++) S[c] += (double)kernel[i * 3u + c];
    for (int c = 0; c < 3; c++) if (!(S[c] > 0.0)) return "kernel channel sums to nothing";
    for (size_t i = 0; i < n; i++) for (int c = 0; c < 3; c++) out[i * 3u + c] = (float)((double)kernel[i * 3u + c] / S[c]);
    return nullptr;
}

// vk_psf_star (include/vecchio_amd.h): the formula is the header's.  Not bit-pinned (it uses libm).
inline void psf_star(uint32_t K, uint32_t streaks, float rotation, float sharpness, float chroma, float *out) {
    const int r = (int)((K - 1u) / 2u);
    const double R = (double)(r > 0 ? r : 1);
    for (int c = 0; c < 3; c++) {
        const double g = 1.0 + (double)chroma * (double)(c - 1);         // the radial scale of the channel
        double S = 0.0;
        for (int y = -r; y <= r; y++) {
            for (int x = -r; x <= r; x++) {
                const double d = sqrt((double)(x * x + y * y)) / g;
                double v = exp(-0.5 * d * d);                            // the core
                if (streaks > 0u && d > 0.0) {
                    const double th = atan2((double)y, (double)x) - (double)rotation;
                    const double a = fabs(cos(0.5 * (double)streaks * th));
                    const double fall = 1.0 - d / R;
                    if (fall > 0.0) v += 0.25 * pow(a, (double)sharpness) * fall * fall / (1.0 + d);
                }
                out[((size_t)(y + r) * K + (size_t)(x + r)) * 3u + (size_t)c] = (float)v;
                S += v;
            }
        }
        for (size_t i = 0; i < (size_t)K * K; i++) out[i * 3u + (size_t)c] = (float)((double)out[i * 3u + (size_t)c] / S);
    }
}

// ---- the whole operator on the host (tests/emu): the definition run literally on std::vector planes ---------------------------------

// a 1-D transform of every line of a Px x Py plane along x (axis 0) or y (axis 1), in place: bit reversal, then the m stages
inline void psf_host_fft_axis(PsfC *a, uint32_t Px, uint32_t Py, uint32_t axis, bool inverse, const PsfC *T) {
    const uint32_t N = axis ? Py : Px, lines = axis ? Px : Py, m = psf_log2(N);
    const size_t step = axis ? Px : 1u, line_step = axis ? 1u : Px;
    for (uint32_t l = 0; l < lines; l++) {
        PsfC *v = a + (size_t)l * line_step;
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t j = psf_rev(i, m);
            if (i < j) { const PsfC t = v[i * step]; v[i * step] = v[j * step]; v[j * step] = t; }
        }
        for (uint32_t s = 1; s <= m; s++) {
            for (uint32_t i = 0; i < N / 2u; i++) {
                uint32_t p, half, wk;
                psf_butterfly_at(i, s, m, p, half, wk);
                psf_butterfly(v[p * step], v[(p + half) * step], T[wk], inverse);
            }
        }
    }
}

// FFT2 or IFFT2 of one plane: rows along x, then columns along y; the inverse ends with the one multiplication by 1 / (Px Py) when
// `scale` is set
inline void psf_host_fft2(PsfC *a, uint32_t Px, uint32_t Py, bool inverse, bool scale) {
    const std::vector<PsfC> Tx = psf_twiddles(Px), Ty = psf_twiddles(Py);
    psf_host_fft_axis(a, Px, Py, 0u, inverse, Tx.data());
    psf_host_fft_axis(a, Px, Py, 1u, inverse, Ty.data());
    if (inverse && scale) {
        const float sc = 1.0f / ((float)Px * (float)Py);
        for (size_t i = 0; i < (size_t)Px * Py; i++) { a[i].re *= sc; a[i].im *= sc; }
    }
}

// out = the operator on a W x H frame with a normalised K x K x 3 kernel (out may be in)
inline void psf_host_apply(uint32_t W, uint32_t H, uint32_t K, const float *kernel, float strength, float threshold, const float *in,
                           float *out) {
    const uint32_t Px = psf_pow2(W + K - 1u), Py = psf_pow2(H + K - 1u);
    const size_t n = (size_t)Px * Py;
    const float sc = 1.0f / ((float)Px * (float)Py);
    std::vector<PsfC> F(n), G(n);
    std::vector<float> res((size_t)W * H * 3u);
    for (uint32_t c = 0; c < 3u; c++) {
        for (uint32_t y = 0; y < Py; y++) {
            for (uint32_t x = 0; x < Px; x++) {
                float B[3] = {0.0f, 0.0f, 0.0f};
                if (x < W && y < H) psf_bright(in + ((size_t)y * W + x) * 3u, threshold, B);
                F[(size_t)y * Px + x] = PsfC{B[c], 0.0f};
                G[(size_t)y * Px + x] = PsfC{psf_placed(kernel, K, c, Px, Py, x, y), 0.0f};
            }
        }
        psf_host_fft2(F.data(), Px, Py, false, false);
        psf_host_fft2(G.data(), Px, Py, false, false);
        for (size_t i = 0; i < n; i++) F[i] = psf_mul(F[i], G[i]);
        psf_host_fft2(F.data(), Px, Py, true, false);
        for (uint32_t y = 0; y < H; y++) {
            for (uint32_t x = 0; x < W; x++) {
                const float *I = in + ((size_t)y * W + x) * 3u;
                float B[3];
                psf_bright(I, threshold, B);
                res[((size_t)y * W + x) * 3u + c] = psf_composite(I[c], B[c], F[(size_t)y * Px + x].re, sc, strength);
            }
        }
    }
    for (size_t i = 0; i < res.size(); i++) out[i] = res[i];
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// psf_pad_kernel: the three planes F from the frame: the bright part at x < W, y < H, +0 elsewhere
struct PsfPadArgs {
    const float *in;
    PsfC *F;                       // three planes
    uint32_t W, H, Px, Py;
    float threshold;
};
// psf_place_kernel: the three planes G from the normalised kernel, its centre at (0, 0), wrapped
struct PsfPlaceArgs {
    const float *kernel;           // K x K x 3
    PsfC *G;
    uint32_t K, Px, Py;
};
// psf_bitrev_kernel: every line of `planes` planes along `axis` into bit-reversed order, in place
// psf_stage_kernel: stage s of every line along `axis`, in place
struct PsfStageArgs {
    PsfC *a;
    const PsfC *T;                 // the table of the axis' length
    uint32_t Px, Py, planes, axis, s, inverse;
};
// psf_product_kernel: F = F * G over n values
struct PsfProductArgs {
    PsfC *F;
    const PsfC *G;
    uint64_t n;
};
// psf_scale_kernel: a *= scale over n values (the end of a bare inverse transform)
struct PsfScaleArgs {
    PsfC *a;
    uint64_t n;
    float scale;
};
// psf_composite_kernel: out = I + strength * (re(F) * scale - B) per pixel of the frame
struct PsfCompositeArgs {
    const float *in;
    float *out;
    const PsfC *F;
    uint32_t W, H, Px, Py;
    float scale, strength, threshold;
};
// psf_line_kernel<COL>: whole lines along x (rows) or y (a tile of adjacent columns) through LDS: load (bit-reversed), m stages, store
enum : uint32_t {
    PSF_LOAD_PLANE = 0u,           // from a
    PSF_LOAD_FRAME = 1u,           // rows: the bright part of the frame, +0 at x >= W
    PSF_LOAD_PRODUCT = 2u,         // a * G
    PSF_LOAD_ROWS = 3u,            // columns: from a at y < valid, +0 at y >= valid (rows the row pass skipped)
    PSF_STORE_PLANE = 0u,          // to a
    PSF_STORE_SCALED = 1u,         // to a, times scale
    PSF_STORE_FRAME = 2u,          // columns: the composite into the frame at x < W, y < H; nothing goes back to a
};
struct PsfLineArgs {
    PsfC *a;                       // `planes` planes
    const PsfC *G;                 // PSF_LOAD_PRODUCT
    const PsfC *T;
    const float *in;               // PSF_LOAD_FRAME, PSF_STORE_FRAME
    float *out;                    // PSF_STORE_FRAME
    uint32_t Px, Py, planes;
    uint32_t lines;                // lines a workgroup takes: a power of two, lines * N within the kernel's LDS
    uint32_t count;                // lines to transform: rows 0 .. count - 1 (the rest are skipped) or columns 0 .. Px - 1
    uint32_t valid;                // PSF_LOAD_ROWS
    uint32_t W, H;
    uint32_t load, store, inverse;
    float scale, strength, threshold;
};

void launch_psf_pad(const PsfPadArgs &A);
void launch_psf_place(const PsfPlaceArgs &A);
void launch_psf_bitrev(const PsfStageArgs &A);
void launch_psf_stage(const PsfStageArgs &A);
void launch_psf_product(const PsfProductArgs &A);
void launch_psf_scale(const PsfScaleArgs &A);
void launch_psf_composite(const PsfCompositeArgs &A);
void launch_psf_line(const PsfLineArgs &A, bool col);
// the lines a workgroup of the line kernel takes for a length-N line
inline uint32_t psf_line_tile(uint32_t N, bool col, uint32_t count) {
    uint32_t l = (col ? PSF_COL_CAP : PSF_ROW_CAP) / N;
    const uint32_t cap = col ? PSF_COL_MAX_LINES : PSF_ROW_MAX_LINES;
    if (l > cap) l = cap;
    while (l > 1u && l / 2u >= count) l /= 2u;
    return l ? l : 1u;
}
#endif

#endif
