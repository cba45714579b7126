// emu_occlusion.cpp — TEST TOOL: occlusion queries (vk_trace_occluded) on the host: vk_trace.h occluded_ray over a batch, on the tree view,
// with the lineariser and the choice of F exactly as emu_rays.cpp has them.  occluded[i] answers rays[i], which is ray first_index + i
// of the caller's batch.  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_occ_err;

template <uint32_t F>
static void occlusion_run(const DScene &S, const GlobalMem &M, uint64_t seed, uint64_t first_index, const vk_ray *rays, uint64_t n,
    uint8_t *occluded) {
    for (uint64_t i = 0; i < n; i++) {
        const vk_ray &r = rays[i];
        Lane L;
        occluded[i] = occluded_ray<F, GlobalMem>(L, S, M, v3(r.origin[0], r.origin[1], r.origin[2]),
                                                 v3(r.direction[0], r.direction[1], r.direction[2]), r.time, r.tmax,
                                                 ray_seed(seed, first_index + i)) ? 1u : 0u;
    }
}

extern "C" {

const char *emu_occlusion_last_error() { return g_occ_err.c_str(); }

int emu_occlusion(const vk_scene_desc *desc, uint64_t seed, uint64_t first_index, const vk_ray *rays, uint64_t n, uint8_t *occluded,
    uint32_t *features_out) {
    if (n != 0u && (!rays || !occluded)) { g_occ_err = "null rays or occluded"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_occ_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        if (features_out) *features_out = LS.features;
        with_features(LS.features, [&](auto f) { occlusion_run<decltype(f)::value>(S, M, seed, first_index, rays, n, occluded); });
    });
}

}  // extern "C"
