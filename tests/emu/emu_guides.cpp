// emu_guides.cpp — TEST TOOL: the specular guides (vk_render_guides) on the host: vk_trace.h guide_sample on the tree as handed over
// (retree 0: the tree vk_api.hip aov_view promises), F chosen as the launcher chooses it.  Built into tests/emu's library only.
// mode 0, per sample: out[(pixel * n + k) * 10 + ..] = albedo3, normal3, depth, hit (0/1), dropped (0/1), bounces of sample
//   first_sample + k, as guide_sample returned them (a dropped sample's values too).
// mode 1, the window [first_sample, first_sample + n) aggregated in specular_guides_kernel's order (vk_kernels.h):
//   out[pixel * 9 + ..] = albedo3, normal3, depth, coverage, bounces.
// Pixels outside the call's tile partition are left as they are.
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

#include "../../vecchio_amd/csrc/vk_linearize.h"
#include "../../vecchio_amd/csrc/vk_trace.h"

using namespace vkd;

static thread_local std::string g_guides_err;

template <uint32_t F>
static void guides_pixel(const DScene &S, const GlobalMem &M, const RenderConsts &C, uint32_t max_bounces, float fuzz_max, uint32_t x,
    uint32_t y, uint32_t first_sample, uint32_t n, int mode, float *out) {
    const size_t pix = (size_t)y * C.width + x;
    V3 sa = v3s(0.0f), sn = v3s(0.0f);
    float sd = 0.0f;
    uint32_t hits = 0u, sb = 0u;
    for (uint32_t k = 0; k < n; k++) {
        Lane L;
        V3 a, nn; float dp; bool h; uint32_t b;
        const bool kept = guide_sample<F, GlobalMem>(L, S, M, C, max_bounces, fuzz_max, x, y, first_sample + k, a, nn, dp, h, b);
        if (mode == 0) {
            float *o = out + (pix * n + k) * 10;
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = nn.x; o[4] = nn.y; o[5] = nn.z; o[6] = dp; o[7] = h ? 1.0f : 0.0f;
            o[8] = kept ? 0.0f : 1.0f; o[9] = (float)b;
            continue;
        }
        if (!kept) continue;                                   // dropped: counts in n only
        sa = sa + a; sn = sn + nn; sb += b;
        if (h) { sd += dp; hits++; }
    }
    if (mode == 0) return;
    const float fn = (float)n;
    float *o = out + pix * 9;
    o[0] = sa.x / fn; o[1] = sa.y / fn; o[2] = sa.z / fn; o[3] = sn.x / fn; o[4] = sn.y / fn; o[5] = sn.z / fn;
    o[6] = hits ? sd / (float)hits : INFINITY;
    o[7] = (float)hits / fn;
    o[8] = (float)sb / fn;
}

extern "C" {

const char *emu_guides_last_error() { return g_guides_err.c_str(); }

int emu_guides(const vk_scene_desc *desc, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, uint32_t n,
    uint32_t max_bounces, float fuzz_max, int mode, float *out, int n_threads, uint32_t *features_out) {
    if (!out || n == 0u || (uint64_t)first_sample + n > 0xFFFFFFFFull) { g_guides_err = "bad sample window / null output"; return VK_ERR_BAD_ARG; }
    if (max_bounces > 8u || !(fuzz_max >= 0.0f) || !(fuzz_max < INFINITY)) { g_guides_err = "bad guide parameters"; return VK_ERR_BAD_ARG; }
    LinearScene LS;
    LinearizeOptions opt;
    opt.retree = 0;
    int st = linearize(desc, LS, g_guides_err, opt);
    if (st != VK_OK) return st;
    DScene S = LS.host_view();
    if (!is_plain_tree_view(S) || S.tie_rank) {
        g_guides_err = "the tree as handed over came with a rebuilt form's gates"; return VK_ERR_BAD_ARG; }
    GlobalMem M{S.items, S.spheres, S.sphere_mat, S.boxes};
    RenderConsts C;
    C.cam = *cam;
    C.width = p->width; C.height = p->height; C.spp = n; C.max_depth = 0u;
    C.seed = p->seed; C.integrator = p->integrator; C.background = p->background;
    C.bg[0] = p->background_color[0]; C.bg[1] = p->background_color[1]; C.bg[2] = p->background_color[2];
    if (features_out) *features_out = LS.features;
    const bool lean = LS.features == 0u;
    if (n_threads < 1) n_threads = 1;
    const uint32_t tiles_x = (p->width + 7) / 8, tiles_y = (p->height + 7) / 8, world = p->tile_world ? p->tile_world : 1;
    std::atomic<uint32_t> next_tile(0);
    auto worker = [&]() {
        for (;;) {
            uint32_t tile = next_tile.fetch_add(1);
            if (tile >= tiles_x * tiles_y) break;
            if (tile % world != p->tile_rank % world) continue;
            const uint32_t x0 = (tile % tiles_x) * 8, y0 = (tile / tiles_x) * 8;
            for (uint32_t y = y0; y < y0 + 8 && y < p->height; y++)
                for (uint32_t x = x0; x < x0 + 8 && x < p->width; x++) {
                    if (lean) guides_pixel<0u>(S, M, C, max_bounces, fuzz_max, x, y, first_sample, n, mode, out);
                    else guides_pixel<(uint32_t)VKF_ALL_SCENE>(S, M, C, max_bounces, fuzz_max, x, y, first_sample, n, mode, out);
                }
        }
    };
    std::vector<std::thread> ths;
    for (int t = 1; t < n_threads; t++) ths.emplace_back(worker);
    worker();
    for (auto &t : ths) t.join();
    return VK_OK;
}

}  // extern "C"
