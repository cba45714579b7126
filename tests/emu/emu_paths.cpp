// emu_paths.cpp — TEST TOOL: the trace step of a path batch (vk_paths_step) on the host: vk_trace.h trace_path on the tree view vk_api.hip
// aov_view promises, F chosen as the launcher chooses it, the provenance tables the lineariser filled.  hits[i] answers rays[i] on the
// stream of states[i], whose counter is advanced by what a ConstantMedium drew.  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_paths_err;

template <uint32_t F>
static void paths_run(const DScene &S, const GlobalMem &M, const DProvenance &P, const vk_ray *rays, vk_path_state *states, uint64_t n,
    vk_hit *hits) {
    static_assert(sizeof(vk_ray) == 32 && sizeof(vk_hit) == 64 && sizeof(vk_path_state) == 48, "the words");
    for (uint64_t i = 0; i < n; i++) {
        uint32_t ray[8], st[12], w[16];
        memcpy(ray, &rays[i], sizeof(ray)); memcpy(st, &states[i], sizeof(st));
        st[7] = trace_path<F, GlobalMem>(S, M, P, ray, st + 4, st + 8, w);
        memcpy(&states[i], st, sizeof(st)); memcpy(&hits[i], w, sizeof(w));
    }
}

extern "C" {

const char *emu_paths_trace_last_error() { return g_paths_err.c_str(); }

int emu_paths_trace(const vk_scene_desc *desc, const vk_ray *rays, vk_path_state *states, uint64_t n, vk_hit *hits, uint32_t *features_out) {
    if (n != 0u && (!rays || !states || !hits)) { g_paths_err = "null rays, states or hits"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_paths_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        const DProvenance P = LS.host_provenance();
        if (features_out) *features_out = LS.features;
        with_features(LS.features, [&](auto f) { paths_run<decltype(f)::value>(S, M, P, rays, states, n, hits); });
    });
}

}  // extern "C"
