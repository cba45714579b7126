// emu_nlm.cpp — TEST TOOL: the non-local-means filter's per-pixel code on the host.  Prepare and the filter of one pixel are the kernels'
// own — vk_nlm.h nlm_prepare_pixel and nlm_filter_pixel, built here with g++ — run over every pixel of an image.  Built into tests/emu's
// library only.
#include <vector>

#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_nlm.h"

static thread_local std::string g_nlm_err;

extern "C" {

const char *emu_nlm_last_error() { return g_nlm_err.c_str(); }

// color, stderr3, albedo (may be null): width * height * 3 floats, y up; planes: [4][3][width * height] floats — I, V, Vf, a
int emu_nlm_prepare(const float *color, const float *stderr3, const float *albedo, uint32_t width, uint32_t height, float albedo_floor,
                    float *planes) {
    if (!color || !stderr3 || !planes) { g_nlm_err = "null argument"; return VK_ERR_BAD_ARG; }
    const size_t n = (size_t)width * height;
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            float I[3], V[3], Vf[3], a[3];
            nlm_prepare_pixel(color, stderr3, albedo, albedo_floor, (int)width, (int)height, (int)x, (int)y, I, V, Vf, a);
            const size_t p = (size_t)y * width + x;
            for (int c = 0; c < 3; c++) {
                planes[c * n + p] = I[c]; planes[(3 + c) * n + p] = V[c]; planes[(6 + c) * n + p] = Vf[c]; planes[(9 + c) * n + p] = a[c];
            }
        }
    return VK_OK;
}

// the whole filter: prepare, then every pixel; out and stderr3_out (may be null): width * height * 3 floats
int emu_nlm_filter(const float *color, const float *stderr3, const float *albedo, uint32_t width, uint32_t height, uint32_t R, uint32_t F,
                   float k, float alpha, float albedo_floor, float *out, float *stderr3_out) {
    if (!color || !stderr3 || !out) { g_nlm_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (R < 1u || R > NLM_MAX_R || F > NLM_MAX_F) { g_nlm_err = "R or F out of range"; return VK_ERR_BAD_ARG; }
    const size_t n = (size_t)width * height;
    std::vector<float> planes(12u * n);
    const int rc = emu_nlm_prepare(color, stderr3, albedo, width, height, albedo_floor, planes.data());
    if (rc != VK_OK) return rc;
    NlmPlanes P;
    P.I = planes.data(); P.V = planes.data() + 3u * n; P.Vf = planes.data() + 6u * n; P.a = planes.data() + 9u * n;
    P.width = width; P.height = height;
    const float kk = k * k;
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            float o[3], se[3];
            nlm_filter_pixel(P, (int)x, (int)y, (int)R, (int)F, alpha, kk, o, se);
            const size_t p = (size_t)y * width + x;
            for (int c = 0; c < 3; c++) {
                out[p * 3 + c] = o[c];
                if (stderr3_out) stderr3_out[p * 3 + c] = se[c];
            }
        }
    return VK_OK;
}

}  // extern "C"
