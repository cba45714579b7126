// emu_shade.cpp — TEST TOOL: shade queries (vk_shade_hits) on the host: vk_trace.h shade_hit on the tree view vk_api.hip aov_view promises,
// with the everything-variant the launcher always takes (plus the integrator's bit), the material count the description's.  out[i]
// answers (rays[i], hits[i], states[i]).  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_shade_err;

template <uint32_t F>
static void shade_run(const DScene &S, const GlobalMem &M, const RenderConsts &C, uint32_t n_materials, const vk_ray *rays,
    const vk_hit *hits, const vk_path_state *states, uint64_t n, vk_shaded *out) {
    static_assert(sizeof(vk_ray) == 32 && sizeof(vk_hit) == 64 && sizeof(vk_path_state) == 48 && sizeof(vk_shaded) == 96, "the words");
    for (uint64_t i = 0; i < n; i++) {
        uint32_t ray[8], hit[16], st[12], w[24];
        memcpy(ray, &rays[i], sizeof(ray)); memcpy(hit, &hits[i], sizeof(hit)); memcpy(st, &states[i], sizeof(st));
        shade_hit<F, GlobalMem>(S, M, C, n_materials, ray, hit, st, w);
        memcpy(&out[i], w, sizeof(w));
    }
}

extern "C" {

const char *emu_shade_last_error() { return g_shade_err.c_str(); }

int emu_shade(const vk_scene_desc *desc, const vk_shade_params *sp, const vk_ray *rays, const vk_hit *hits, const vk_path_state *states,
    uint64_t n, vk_shaded *out, uint32_t *features_out) {
    if (!sp || (n != 0u && (!rays || !hits || !states || !out))) { g_shade_err = "null params, rays, hits, states or out"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_shade_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        if (features_out) *features_out = LS.features;
        RenderConsts C;
        memset(&C, 0, sizeof(C));
        C.spp = 1u; C.max_depth = sp->max_depth; C.integrator = sp->integrator; C.background = sp->background;
        C.bg[0] = sp->background_color[0]; C.bg[1] = sp->background_color[1]; C.bg[2] = sp->background_color[2];
        const uint32_t nm = (uint32_t)LS.materials.size();
        if (sp->integrator == VK_INTEGRATOR_PDF)
            shade_run<(uint32_t)VKF_ALL_SCENE | (uint32_t)VKF_INTEG_PDF>(S, M, C, nm, rays, hits, states, n, out);
        else
            shade_run<(uint32_t)VKF_ALL_SCENE>(S, M, C, nm, rays, hits, states, n, out);
    });
}

}  // extern "C"
