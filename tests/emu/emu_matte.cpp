// emu_matte.cpp — TEST TOOL: ID mattes (vk_render_mattes) on the host: vk_matte.h matte_sample, matte_insert and matte_sort, built here
// with g++, on the tree view vk_api.hip aov_view promises (emu_query.h), F chosen as the launcher chooses it, the provenance tables the
// lineariser filled.  Built into tests/emu's library only.
// mode 0, per sample: ids[(pixel * n + k)] = the id of sample first_sample + k.
// mode 1, the window's table in matte_kernel's order: ids[pixel * ranks + r], counts[pixel * ranks + r], overflow[pixel].
// Pixels outside the call's tile partition are left as they are.
#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_matte.h"

static thread_local std::string g_matte_err;

template <uint32_t F>
static void matte_pixel(const DScene &S, const GlobalMem &M, const DProvenance &P, const RenderConsts &C, uint32_t x, uint32_t y,
    uint32_t first_sample, uint32_t n, uint32_t kind, uint32_t ranks, int mode, uint32_t *ids, uint32_t *counts, uint32_t *overflow) {
    const size_t pix = (size_t)y * C.width + x;
    MatteTable T;
    matte_clear(T);
    for (uint32_t k = 0; k < n; k++) {
        Lane L;
        const uint32_t id = matte_sample<F, GlobalMem>(L, S, M, P, C, x, y, first_sample + k, kind);
        if (mode == 0) ids[pix * n + k] = id;
        else matte_insert(T, ranks, id, 1u);
    }
    if (mode == 0) return;
    matte_sort(T);
    for (uint32_t r = 0; r < ranks; r++) { ids[pix * ranks + r] = T.id[r]; counts[pix * ranks + r] = T.cnt[r]; }
    if (overflow) overflow[pix] = T.overflow;
}

extern "C" {

const char *emu_matte_last_error() { return g_matte_err.c_str(); }

int emu_matte(const vk_scene_desc *desc, const vk_camera *cam, const vk_render_params *p, uint32_t first_sample, uint32_t n, uint32_t kind,
    uint32_t ranks, int mode, uint32_t *ids, uint32_t *counts, uint32_t *overflow, uint32_t *features_out) {
    if (!ids || (mode != 0 && !counts) || n == 0u || (uint64_t)first_sample + n > 0xFFFFFFFFull) {
        g_matte_err = "bad sample window / null output"; return VK_ERR_BAD_ARG; }
    if (kind > (uint32_t)VK_MATTE_MATERIAL || ranks < 1u || ranks > VK_MATTE_MAX_RANKS) { g_matte_err = "bad matte parameters"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_matte_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        const DProvenance P = LS.host_provenance();
        RenderConsts C;
        memset(&C, 0, sizeof(C));
        C.cam = *cam;
        C.width = p->width; C.height = p->height; C.spp = n; C.seed = p->seed;
        if (features_out) *features_out = LS.features;
        const uint32_t tiles_x = (p->width + 7) / 8, tiles_y = (p->height + 7) / 8, world = p->tile_world ? p->tile_world : 1;
        with_features(LS.features, [&](auto f) {
            for (uint32_t tile = p->tile_rank; tile < tiles_x * tiles_y; tile += world) {
                const uint32_t x0 = (tile % tiles_x) * 8, y0 = (tile / tiles_x) * 8;
                for (uint32_t y = y0; y < y0 + 8 && y < p->height; y++)
                    for (uint32_t x = x0; x < x0 + 8 && x < p->width; x++)
                        matte_pixel<decltype(f)::value>(S, M, P, C, x, y, first_sample, n, kind, ranks, mode, ids, counts, overflow);
            }
        });
    });
}

// matte_insert and matte_sort alone: the table of `n` ids taken in order
int emu_matte_table(const uint32_t *sample_ids, uint32_t n, uint32_t ranks, uint32_t *ids, uint32_t *counts, uint32_t *overflow) {
    if (!sample_ids || !ids || !counts || !overflow || ranks < 1u || ranks > VK_MATTE_MAX_RANKS) {
        g_matte_err = "bad matte table arguments"; return VK_ERR_BAD_ARG; }
    MatteTable T;
    matte_clear(T);
    for (uint32_t k = 0; k < n; k++) matte_insert(T, ranks, sample_ids[k], 1u);
    matte_sort(T);
    for (uint32_t r = 0; r < ranks; r++) { ids[r] = T.id[r]; counts[r] = T.cnt[r]; }
    *overflow = T.overflow;
    return VK_OK;
}

}  // extern "C"
