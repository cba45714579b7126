// emu_psf.cpp — TEST TOOL: the point-spread stage on the host.  The bright part, the butterfly, the product and the composite are the
// kernels' own — vk_psf.h psf_bright, psf_butterfly, psf_mul and psf_composite, built here with g++ — run over whole planes in the
// definition's order (vk_psf.h psf_host_apply), and the library's tables, normalisation and star.  Built into tests/emu's library only.
#include <string>
#include <vector>

#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_psf.h"

static thread_local std::string g_psf_err;

extern "C" {

const char *emu_psf_last_error() { return g_psf_err.c_str(); }

// the table of a length N: N / 2 (re, im) pairs
int emu_psf_twiddles(uint32_t N, float *out) {
    if (!out || N < 2u || N > PSF_MAX_N || (N & (N - 1u))) { g_psf_err = "bad argument"; return VK_ERR_BAD_ARG; }
    const std::vector<PsfC> T = psf_twiddles(N);
    for (size_t k = 0; k < T.size(); k++) { out[2 * k] = T[k].re; out[2 * k + 1] = T[k].im; }
    return VK_OK;
}

// the kernel as a load normalises it; VK_ERR_BAD_ARG with the load's reason for one it refuses
int emu_psf_normalise(uint32_t K, const float *kernel, float *out) {
    if (!kernel || !out || K < PSF_MIN_K || K > PSF_MAX_K || !(K & 1u)) { g_psf_err = "bad argument"; return VK_ERR_BAD_ARG; }
    if (const char *why = psf_normalise(K, kernel, out)) { g_psf_err = why; return VK_ERR_BAD_ARG; }
    return VK_OK;
}

// one bare 2-D transform of Px x Py (re, im) pairs in place; the inverse with its closing multiplication
int emu_psf_fft2(uint32_t Px, uint32_t Py, uint32_t inverse, float *data) {
    if (!data) { g_psf_err = "null argument"; return VK_ERR_BAD_ARG; }
    for (uint32_t N : {Px, Py}) if (N < 2u || N > PSF_MAX_N || (N & (N - 1u))) { g_psf_err = "bad size"; return VK_ERR_BAD_ARG; }
    psf_host_fft2(reinterpret_cast<PsfC *>(data), Px, Py, inverse != 0u, true);
    return VK_OK;
}

// in, out: width * height * 3 floats, y up; kernel: K * K * 3 floats as the caller would load it; out may be in
int emu_psf_apply(const float *in, uint32_t width, uint32_t height, uint32_t K, const float *kernel, float strength, float threshold,
                  float *out) {
    if (!in || !out || !kernel || !width || !height) { g_psf_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (K < PSF_MIN_K || K > PSF_MAX_K || !(K & 1u)) { g_psf_err = "K must be odd and in 3..1023"; return VK_ERR_BAD_ARG; }
    if (width + K - 1u > PSF_MAX_N || height + K - 1u > PSF_MAX_N) { g_psf_err = "padded size exceeds 4096"; return VK_ERR_BAD_ARG; }
    std::vector<float> norm((size_t)K * K * 3u);
    if (const char *why = psf_normalise(K, kernel, norm.data())) { g_psf_err = why; return VK_ERR_BAD_ARG; }
    psf_host_apply(width, height, K, norm.data(), strength, threshold, in, out);
    return VK_OK;
}

}  // extern "C"
