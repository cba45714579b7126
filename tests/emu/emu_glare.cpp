// emu_glare.cpp — TEST TOOL: the glare stage's per-pixel code on the host.  The bright part, a pixel of a down pass, of an up pass and of
// the composite are the kernels' own — vk_glare.h glare_down_pixel, glare_up_pixel and glare_composite_pixel, built here with g++ — run
// over every pixel of every level, in the plain form's order.  Built into tests/emu's library only.
#include <vector>

#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_glare.h"

static thread_local std::string g_glare_err;

extern "C" {

const char *emu_glare_last_error() { return g_glare_err.c_str(); }

// the weights c_0 .. c_{levels-1} as the library computes them
int emu_glare_weights(uint32_t levels, float falloff, float *c) {
    if (!c || levels < 1u || levels > GLARE_MAX_LEVELS) { g_glare_err = "bad argument"; return VK_ERR_BAD_ARG; }
    float all[GLARE_MAX_LEVELS];
    glare_weights(levels, falloff, all);
    for (uint32_t l = 0; l < levels; l++) c[l] = all[l];
    return VK_OK;
}

// the first level the fused form's tail takes over from, and the kernels one apply launches in `form`
uint32_t emu_glare_tail_level(uint32_t width, uint32_t height) { return glare_tail_level(glare_dims(width, height)); }
uint32_t emu_glare_launch_count(uint32_t width, uint32_t height, uint32_t levels, uint32_t form) {
    return glare_launch_count(width, height, levels, form);
}

// in, out: width * height * 3 floats, y up; out may be in
int emu_glare_apply(const float *in, uint32_t width, uint32_t height, uint32_t levels, float strength, float falloff, float threshold,
                    float *out) {
    if (!in || !out || !width || !height) { g_glare_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (levels < 1u || levels > GLARE_MAX_LEVELS) { g_glare_err = "levels out of range"; return VK_ERR_BAD_ARG; }
    const uint32_t L = levels;
    const GlareDims d = glare_dims(width, height);
    float c[GLARE_MAX_LEVELS];
    glare_weights(L, falloff, c);
    std::vector<std::vector<float>> B(L), A(L);
    for (uint32_t l = 0; l + 1u < L; l++) {
        const int dw = d.w[l + 1], dh = d.h[l + 1];
        B[l + 1].resize((size_t)dw * dh * 3u);
        for (int Y = 0; Y < dh; Y++)
            for (int X = 0; X < dw; X++) {
                float *o = &B[l + 1][((size_t)Y * dw + X) * 3u];
                if (l == 0u) glare_down_pixel<true>(in, d.w[0], d.h[0], threshold, X, Y, o);
                else glare_down_pixel<false>(B[l].data(), d.w[l], d.h[l], threshold, X, Y, o);
            }
    }
    for (uint32_t l = L - 1u; l-- > 1u;) {
        const bool top = l + 2u == L;
        const float *src = top ? B[l + 1].data() : A[l + 1].data();
        A[l].resize((size_t)d.w[l] * d.h[l] * 3u);
        for (int y = 0; y < d.h[l]; y++)
            for (int x = 0; x < d.w[l]; x++) {
                float up[3];
                glare_up_pixel(src, d.w[l + 1], d.h[l + 1], top ? c[L - 1u] : 1.0f, x, y, up);
                const size_t p = ((size_t)y * d.w[l] + x) * 3u;
                for (int k = 0; k < 3; k++) A[l][p + k] = c[l] * B[l][p + k] + up[k];
            }
    }
    const float *src = L >= 3u ? A[1].data() : (L == 2u ? B[1].data() : nullptr);
    const float scale = L == 2u ? c[1] : 1.0f;
    for (int y = 0; y < d.h[0]; y++)
        for (int x = 0; x < d.w[0]; x++) {
            const size_t p = ((size_t)y * d.w[0] + x) * 3u;
            const float I[3] = {in[p], in[p + 1], in[p + 2]};
            float up[3] = {0.0f, 0.0f, 0.0f}, o[3];
            if (src) glare_up_pixel(src, d.w[1], d.h[1], scale, x, y, up);
            glare_composite_pixel(I, threshold, c[0], strength, src != nullptr, up, o);
            out[p] = o[0]; out[p + 1] = o[1]; out[p + 2] = o[2];
        }
    return VK_OK;
}

}  // extern "C"
