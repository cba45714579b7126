// emu_splat.cpp — TEST TOOL: vk_splat_deposit on the host.  The filter's coefficients, a sample's position and its footprint are the
// kernels' own — vk_splat.h splat_filter_for, splat_position_* and splat_weights, built here with g++ —; the clamp, the conversion and
// the sums are plain C++ as emu_film_deposit's are.  Built into tests/emu's library only.
#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_splat.h"

static thread_local std::string g_splat_err;

extern "C" {

const char *emu_splat_last_error() { return g_splat_err.c_str(); }

// sums4: width * height * 4 values (r, g, b, weight), added to; counters: deposited, dropped, clamped, skipped, contributions, added to;
// positions: null or 2 * n floats
int emu_splat_deposit(const vk_path_state *states, const uint32_t *status, uint64_t n, const float *positions, uint32_t width,
    uint32_t height, uint32_t samples_per_pixel, const vk_splat_params *sp, long long *sums4, uint64_t counters[5]) {
    if ((n != 0u && (!states || !status)) || !sp || !sums4 || !counters || samples_per_pixel == 0u || width == 0u || height == 0u) {
        g_splat_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (sp->filter > (uint32_t)VK_SPLAT_MITCHELL || !(sp->radius >= 0.5f && sp->radius <= 2.0f)) {
        g_splat_err = "unknown filter or radius outside [0.5, 2]"; return VK_ERR_BAD_ARG; }
    const bool mitchell = sp->filter == (uint32_t)VK_SPLAT_MITCHELL;
    const SplatFilter P = splat_filter_for(sp->filter, sp->radius, mitchell ? sp->b : 0.0f, mitchell ? sp->c : 0.0f);
    const float scale = 67108864.0f;                    // 2^26
    const uint32_t side = (uint32_t)std::ceil(2.0f * sp->radius);
    float clampv = 1.3e11f / (float)(samples_per_pixel * side * side);
    if (!(clampv < 1.0e10f)) clampv = 1.0e10f;
    for (uint64_t i = 0; i < n; i++) {
        const bool retired = status[i] == (uint32_t)VK_SHADE_MISS || status[i] == (uint32_t)VK_SHADE_ENDED || status[i] == (uint32_t)VK_PATHS_CULLED;
        uint32_t ix = 0, iy = 0;
        float fx = 0.0f, fy = 0.0f;
        const bool placed = retired && (positions
            ? splat_position_given(positions[2 * i], positions[2 * i + 1], width, height, ix, iy, fx, fy)
            : splat_position_of_state(states[i].seed, states[i].pixel, states[i].sample, width, height, ix, iy, fx, fy));
        if (!placed) { counters[3]++; continue; }
        float a[3] = {states[i].acc[0], states[i].acc[1], states[i].acc[2]};
        if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) { counters[1]++; continue; }
        const float big = std::fmax(std::fmax(std::fabs(a[0]), std::fabs(a[1])), std::fabs(a[2]));
        const bool large = big > 31.999f;
        if (large && big > clampv) counters[2]++;
        if (large) for (float &v : a) v = std::fmin(std::fmax(v, -clampv), clampv);
        counters[0]++;
        SplatFoot F;
        counters[4] += splat_weights(P, ix, fx, iy, fy, width, height, F);
        for (int ky = 0; ky < 5; ky++)
            for (int kx = 0; kx < 5; kx++) {
                if (!((F.my >> ky) & 1u) || !((F.mx >> kx) & 1u)) continue;
                const float w = F.wx[kx] * F.wy[ky];
                long long *s = sums4 + ((size_t)(iy + ky - 2) * width + (size_t)(ix + kx - 2)) * 4u;
                for (int c = 0; c < 3; c++) s[c] += (long long)((w * a[c]) * scale);      // exact scaling; the cast truncates toward zero
                s[3] += (long long)(w * scale);
            }
    }
    return VK_OK;
}

}  // extern "C"
