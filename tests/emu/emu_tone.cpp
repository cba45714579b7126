// emu_tone.cpp — TEST TOOL: the display transform's per-pixel code on the host.  The classification of a pixel for the histogram, the
// curves and the three transfers are the kernels' own — vk_tone.h tone_classify and tone_pixel<curve, table, dither>, built here with
// g++, one instance per combination as the device builds them.  Built into tests/emu's library only.
#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_tone.h"

static thread_local std::string g_tone_err;

namespace {

template <uint32_t CURVE, bool TABLE, bool DITHER>
void encode_all(const float *rgb, uint32_t width, uint32_t height, const float *h, float E, float p, uint64_t seed, uint8_t *out) {
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const uint32_t pixel = y * width + x;
            uint32_t code[3];
            tone_pixel<CURVE, TABLE, DITHER>(rgb + (size_t)pixel * 3u, h, E, p, seed, pixel, code);
            uint8_t *o = out + ((size_t)(height - 1u - y) * width + x) * 3u;
            o[0] = (uint8_t)code[0]; o[1] = (uint8_t)code[1]; o[2] = (uint8_t)code[2];
        }
}

template <uint32_t CURVE>
void encode_curve(bool table, bool dither, const float *rgb, uint32_t width, uint32_t height, const float *h, float E, float p, uint64_t seed,
                  uint8_t *out) {
    if (!table) encode_all<CURVE, false, false>(rgb, width, height, h, E, p, seed, out);
    else if (!dither) encode_all<CURVE, true, false>(rgb, width, height, h, E, p, seed, out);
    else encode_all<CURVE, true, true>(rgb, width, height, h, E, p, seed, out);
}

}  // namespace

extern "C" {

const char *emu_tone_last_error() { return g_tone_err.c_str(); }

// rgb: n * 3 floats; bins: 640 words and counters: 4 (binned, below, above, nonfinite), both added to
int emu_tone_histogram(const float *rgb, uint64_t n, uint32_t *bins, uint64_t *counters) {
    if (!rgb || !bins || !counters) { g_tone_err = "null argument"; return VK_ERR_BAD_ARG; }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t w = tone_classify(rgb[i * 3u], rgb[i * 3u + 1u], rgb[i * 3u + 2u]);
        if (w < TONE_BINS) { bins[w]++; counters[TONE_BINNED]++; }
        else counters[w - TONE_BINS]++;
    }
    return VK_OK;
}

// h(white) as vk_tone_encode computes it on the host
float emu_tone_hable(float v) { return tone_hable(v); }

// rgb: width * height * 3 floats, y up; table: the 510 thresholds (table transfers) or null; E and p as the host hands them to the kernel
// (p: REINHARD white * white, HABLE h(white)); out: width * height * 3 bytes, row 0 the top
int emu_tone_encode(const float *rgb, uint32_t width, uint32_t height, uint32_t curve, const float *table, int dither, float E, float p,
                    uint64_t seed, uint8_t *out) {
    if (!rgb || !out) { g_tone_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (dither && !table) { g_tone_err = "dither needs a table"; return VK_ERR_BAD_ARG; }
    const bool t = table != nullptr, d = dither != 0;
    switch (curve) {
        case TONE_CLAMP: encode_curve<TONE_CLAMP>(t, d, rgb, width, height, table, E, p, seed, out); break;
        case TONE_REINHARD: encode_curve<TONE_REINHARD>(t, d, rgb, width, height, table, E, p, seed, out); break;
        case TONE_HABLE: encode_curve<TONE_HABLE>(t, d, rgb, width, height, table, E, p, seed, out); break;
        case TONE_ACES: encode_curve<TONE_ACES>(t, d, rgb, width, height, table, E, p, seed, out); break;
        default: g_tone_err = "unknown curve"; return VK_ERR_BAD_ARG;
    }
    return VK_OK;
}

}  // extern "C"
