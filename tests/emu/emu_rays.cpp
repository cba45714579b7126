// emu_rays.cpp — TEST TOOL: ray queries (vk_trace_rays) on the host: vk_trace.h trace_ray on the tree view vk_api.hip aov_view promises
// (the tree as handed over; under VK_SCENE_FAST_ACCEL the rebuilt tree with its tie table), F chosen as the launcher chooses it, the
// provenance tables the lineariser filled.  hits[i] answers rays[i], which is ray first_index + i of the caller's batch.  Built into
// tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_rays_err;

template <uint32_t F>
static void rays_run(const DScene &S, const GlobalMem &M, const DProvenance &P, uint64_t seed, uint64_t first_index, const vk_ray *rays,
    uint64_t n, vk_hit *hits) {
    for (uint64_t i = 0; i < n; i++) {
        const vk_ray &r = rays[i];
        Lane L;
        RayHit H;
        trace_ray<F, GlobalMem>(L, S, M, P, v3(r.origin[0], r.origin[1], r.origin[2]), v3(r.direction[0], r.direction[1], r.direction[2]),
                                r.time, r.tmax, ray_seed(seed, first_index + i), H);
        uint32_t w[16];
        hit_words(H, w);
        static_assert(sizeof(vk_hit) == sizeof(w), "vk_hit is sixteen words");
        memcpy(&hits[i], w, sizeof(w));
    }
}

extern "C" {

const char *emu_rays_last_error() { return g_rays_err.c_str(); }

int emu_rays(const vk_scene_desc *desc, uint64_t seed, uint64_t first_index, const vk_ray *rays, uint64_t n, vk_hit *hits,
    uint32_t *features_out) {
    if (n != 0u && (!rays || !hits)) { g_rays_err = "null rays or hits"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_rays_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        const DProvenance P = LS.host_provenance();
        if (features_out) *features_out = LS.features;
        with_features(LS.features, [&](auto f) { rays_run<decltype(f)::value>(S, M, P, seed, first_index, rays, n, hits); });
    });
}

}  // extern "C"
