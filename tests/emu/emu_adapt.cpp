// emu_adapt.cpp — TEST TOOL: the top-up of a film's tile run (vk_adapt_begin) on the host.  The index code is the kernel's own,
// vk_adapt.h adapt_locate, on a list and a prefix built here by a plain loop over the tile map; emu_adapt_emit then starts each path
// with vk_trace.h start_sample_core as emu_film_emit does.  Built into tests/emu's library only.
#include <algorithm>
#include <vector>

#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_adapt.h"

static thread_local std::string g_adapt_err;

namespace {

struct HostTiles {
    std::vector<uint32_t> list, prefix;
    AdaptTiles T;
};

// tile_n[t] == 0: tile t is active
void host_tiles(uint32_t width, uint32_t height, const uint32_t *tile_n, HostTiles &H) {
    const uint32_t tiles_x = (width + 7u) / 8u, tiles_y = (height + 7u) / 8u;
    uint32_t px = 0;
    for (uint32_t t = 0; t < tiles_x * tiles_y; t++) {
        if (tile_n[t] != 0u) continue;
        const uint32_t tx = t % tiles_x, ty = t / tiles_x;
        H.list.push_back(t); H.prefix.push_back(px);
        px += std::min(8u, width - 8u * tx) * std::min(8u, height - 8u * ty);
    }
    H.prefix.push_back(px);
    H.list.push_back(0u);                 // (never read: keeps data() non-null with no tile active)
    H.T = AdaptTiles{H.list.data(), H.prefix.data(), (uint32_t)H.list.size() - 1u, width, height, tiles_x,
                     (width % 8u == 0u && height % 8u == 0u) ? 1u : 0u};
}

bool in_run(const HostTiles &H, uint32_t n_samples, uint64_t first, uint64_t m) {
    return n_samples != 0u && first + m <= (uint64_t)H.prefix.back() * n_samples && first + m < (1ull << 32);
}

}  // namespace

extern "C" {

const char *emu_adapt_last_error() { return g_adapt_err.c_str(); }

// the paths of the run over the active tiles: *total = their number
int emu_adapt_total(uint32_t width, uint32_t height, const uint32_t *tile_n, uint32_t n_samples, uint64_t *total) {
    if (!tile_n || !total || width == 0u || height == 0u) { g_adapt_err = "null argument"; return VK_ERR_BAD_ARG; }
    HostTiles H;
    host_tiles(width, height, tile_n, H);
    *total = (uint64_t)H.prefix.back() * n_samples;
    return VK_OK;
}

int emu_adapt_sequence(uint32_t width, uint32_t height, const uint32_t *tile_n, uint32_t n_samples, uint32_t samples_done, uint64_t first,
                       uint64_t m, uint32_t *pixel_out, uint32_t *sample_out) {
    if (!tile_n || !pixel_out || !sample_out || width == 0u || height == 0u) { g_adapt_err = "null argument"; return VK_ERR_BAD_ARG; }
    HostTiles H;
    host_tiles(width, height, tile_n, H);
    if (!in_run(H, n_samples, first, m)) { g_adapt_err = "paths beyond the run"; return VK_ERR_BAD_ARG; }
    for (uint64_t i = 0; i < m; i++) {
        uint32_t x, y, k;
        pixel_out[i] = adapt_locate(H.T, n_samples, (uint32_t)(first + i), x, y, k);
        sample_out[i] = samples_done + k;
    }
    return VK_OK;
}

int emu_adapt_emit(const vk_camera *cam, const vk_render_params *p, const uint32_t *tile_n, uint32_t n_samples, uint32_t samples_done,
                   uint64_t first, uint64_t m, vk_ray *rays, vk_path_state *states, uint32_t *ids) {
    if (!cam || !p || !tile_n || !rays || !states || !ids) { g_adapt_err = "null argument"; return VK_ERR_BAD_ARG; }
    HostTiles H;
    host_tiles(p->width, p->height, tile_n, H);
    if (!in_run(H, n_samples, first, m) || (uint64_t)samples_done + n_samples > p->samples_per_pixel) {
        g_adapt_err = "paths beyond the run, or samples beyond the film's"; return VK_ERR_BAD_ARG; }
    RenderConsts C;
    memset(&C, 0, sizeof(C));
    C.cam = *cam;
    C.width = p->width; C.height = p->height; C.spp = p->samples_per_pixel; C.max_depth = p->max_depth; C.seed = p->seed;
    C.integrator = p->integrator; C.background = p->background;
    C.bg[0] = p->background_color[0]; C.bg[1] = p->background_color[1]; C.bg[2] = p->background_color[2];
    for (uint64_t i = 0; i < m; i++) {
        uint32_t x, y, k;
        adapt_locate(H.T, n_samples, (uint32_t)(first + i), x, y, k);
        Lane L;
        V3 o, d;
        float time;
        start_sample_core(L, C, x, y, samples_done + k, o, d, time);
        vk_ray &r = rays[i];
        r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmax = INFINITY;
        r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z; r.time = time;
        vk_path_state &s = states[i];
        s.thr[0] = L.thr.x; s.thr[1] = L.thr.y; s.thr[2] = L.thr.z; s.depth = L.depth;
        s.acc[0] = L.acc.x; s.acc[1] = L.acc.y; s.acc[2] = L.acc.z; s.counter = L.rng.ctr;
        s.seed = p->seed; s.pixel = L.pixel; s.sample = L.sample;
        ids[i] = (uint32_t)(first + i);
    }
    return VK_OK;
}

}  // extern "C"
