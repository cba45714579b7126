// emu_upsample.cpp — TEST TOOL: guided upsampling's per-pixel code on the host.  The prepare pass and the filter are the kernels' own —
// vk_upsample.h upsample_prepare_pixel and upsample_pixel, built here with g++ — run over every low and every high pixel, the taps'
// records straight from the planes as the plain form reads them.  Built into tests/emu's library only.
#include <vector>

#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_upsample.h"

static thread_local std::string g_upsample_err;

extern "C" {

const char *emu_upsample_last_error() { return g_upsample_err.c_str(); }

// AUTO's form for a pair of sizes, as the library decides it
uint32_t emu_upsample_auto_form(uint32_t w, uint32_t h, uint32_t W, uint32_t H) { return upsample_auto_form(w, h, W, H); }

// the two ratios of one axis as the library computes them: r_s[0] = rx, r_s[1] = sx
int emu_upsample_ratios(uint32_t lo, uint32_t hi, float *r_s) {
    if (!r_s || lo < 2u || hi < lo) { g_upsample_err = "bad argument"; return VK_ERR_BAD_ARG; }
    upsample_ratios(lo, hi, r_s[0], r_s[1]);
    return VK_OK;
}

// The low images (w x h; all but color may be null) and the high guides (W x H; may be null) -> out, stderr3_out (may be null) [W * H *
// 3] and counts[2] = fallback_pixels, empty_pixels.  vk_upsample_load's and vk_upsample_apply's pairing rules.
int emu_upsample_apply(const float *color, const float *stderr3, const float *albedo, const float *normal, const float *depth,
                       uint32_t w, uint32_t h, uint32_t W, uint32_t H, const float *albedo_hi, const float *normal_hi, const float *depth_hi,
                       float sigma_z, uint32_t normal_squarings, float albedo_floor, float *out, float *stderr3_out, uint64_t *counts) {
    if (!color || !out || !counts) { g_upsample_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (w < 2u || h < 2u || w > W || h > H) { g_upsample_err = "sizes outside the rules"; return VK_ERR_BAD_ARG; }
    if ((albedo != nullptr) != (albedo_hi != nullptr)) { g_upsample_err = "albedo must be given at both sizes or at neither"; return VK_ERR_BAD_ARG; }
    if (stderr3_out && !stderr3) { g_upsample_err = "stderr3_out wanted but no stderr3 was loaded"; return VK_ERR_BAD_ARG; }
    const size_t n = (size_t)w * h;
    std::vector<UpRec> P0(n), P1(n), P2(n);
    for (size_t q = 0; q < n; q++) upsample_prepare_pixel(color, stderr3, albedo, normal, depth, albedo_floor, q, P0[q], P1[q], P2[q]);
    uint32_t unused[2] = {0u, 0u};
    UpsampleArgs A = {};
    A.P0 = P0.data(); A.P1 = P1.data(); A.P2 = P2.data();
    A.albedo_hi = albedo_hi; A.normal_hi = normal_hi; A.depth_hi = depth_hi;
    A.out = out; A.stderr3_out = stderr3_out; A.counts = unused;
    A.w = w; A.h = h; A.W = W; A.H = H;
    upsample_ratios(w, W, A.rx, A.sx);
    upsample_ratios(h, H, A.ry, A.sy);
    A.sigma_z = sigma_z; A.albedo_floor = albedo_floor; A.normal_squarings = normal_squarings;
    A.flags = (normal && normal_hi ? UP_NORMAL : 0u) | (depth && depth_hi ? UP_DEPTH : 0u);
    counts[0] = 0u; counts[1] = 0u;
    for (int Y = 0; Y < (int)H; Y++)
        for (int X = 0; X < (int)W; X++) {
            const int what = upsample_pixel(A, X, Y, [&](int tx, int ty, UpRec &q0, UpRec &q1, UpRec &q2) {
                const size_t q = (size_t)ty * w + (size_t)tx;
                q0 = P0[q]; q1 = P1[q]; q2 = P2[q];
            });
            if (what >= 1) counts[0]++;
            if (what == 2) counts[1]++;
        }
    return VK_OK;
}

}  // extern "C"
