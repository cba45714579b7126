// emu_film.cpp — TEST TOOL: the two ends of a film (vk_film_emit, vk_film_deposit) on the host.  emu_film_emit is vk_trace.h
// start_sample_core, the render kernel's camera, filling the rays and states of a window in the id order the header gives;
// emu_film_deposit is the render kernel's finite filter, conversion and sums in plain C++.  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_film_err;

extern "C" {

const char *emu_film_last_error() { return g_film_err.c_str(); }

int emu_film_emit(const vk_camera *cam, const vk_render_params *p, const vk_film_window *win, vk_ray *rays, vk_path_state *states) {
    if (!cam || !p || !win || !rays || !states) { g_film_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (win->width == 0u || win->height == 0u || win->n_samples == 0u || (uint64_t)win->x0 + win->width > p->width ||
        (uint64_t)win->y0 + win->height > p->height || (uint64_t)win->first_sample + win->n_samples > p->samples_per_pixel) {
        g_film_err = "an empty window, or one outside the frame or the samples"; return VK_ERR_BAD_ARG; }
    RenderConsts C;
    memset(&C, 0, sizeof(C));
    C.cam = *cam;
    C.width = p->width; C.height = p->height; C.spp = p->samples_per_pixel; C.max_depth = p->max_depth; C.seed = p->seed;
    C.integrator = p->integrator; C.background = p->background;
    C.bg[0] = p->background_color[0]; C.bg[1] = p->background_color[1]; C.bg[2] = p->background_color[2];
    uint64_t id = 0;
    for (uint32_t y = win->y0; y < win->y0 + win->height; y++)
        for (uint32_t x = win->x0; x < win->x0 + win->width; x++)
            for (uint32_t k = 0; k < win->n_samples; k++, id++) {
                Lane L;
                V3 o, d;
                float time;
                start_sample_core(L, C, x, y, win->first_sample + k, o, d, time);
                vk_ray &r = rays[id];
                r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmax = INFINITY;
                r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.time = time;
                vk_path_state &s = states[id];
                s.thr[0] = L.thr.x; s.thr[1] = L.thr.y; s.thr[2] = L.thr.z; s.depth = L.depth;
                s.acc[0] = L.acc.x; s.acc[1] = L.acc.y; s.acc[2] = L.acc.z; s.counter = L.rng.ctr;
                s.seed = p->seed; s.pixel = L.pixel; s.sample = L.sample;
            }
    return VK_OK;
}

// sums: n_pixels * 3 values, added to; counters: deposited, dropped, clamped, skipped, added to
int emu_film_deposit(const vk_path_state *states, const uint32_t *status, uint64_t n, uint32_t n_pixels, uint32_t samples_per_pixel,
    long long *sums, uint64_t counters[4]) {
    if ((n != 0u && (!states || !status)) || !sums || !counters || samples_per_pixel == 0u) { g_film_err = "null argument"; return VK_ERR_BAD_ARG; }
    const float scale = 67108864.0f;                    // 2^26
    float clampv = 1.3e11f / (float)samples_per_pixel;
    if (!(clampv < 1.0e10f)) clampv = 1.0e10f;
    for (uint64_t i = 0; i < n; i++) {
        const bool retired = status[i] == (uint32_t)VK_SHADE_MISS || status[i] == (uint32_t)VK_SHADE_ENDED || status[i] == (uint32_t)VK_PATHS_CULLED;
        if (!retired || states[i].pixel >= n_pixels) { counters[3]++; continue; }
        const float *a = states[i].acc;
        if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) { counters[1]++; continue; }
        const float big = std::fmax(std::fmax(std::fabs(a[0]), std::fabs(a[1])), std::fabs(a[2]));
        const bool large = big > 31.999f;
        if (large && big > clampv) counters[2]++;
        for (int c = 0; c < 3; c++) {
            float v = a[c];
            if (large) v = std::fmin(std::fmax(v, -clampv), clampv);
            sums[(size_t)states[i].pixel * 3u + c] += (long long)(v * scale);        // exact scaling; the cast truncates toward zero
        }
        counters[0]++;
    }
    return VK_OK;
}

}  // extern "C"
