// emu_probes.cpp — TEST TOOL: probe queries (vk_trace_probes) on the host: vk_trace.h probe_sample and sh9 on the tree view vk_api.hip
// aov_view promises, F chosen as the launcher chooses it (as emu_irradiance.cpp, which see).  samples[(i * samples_per_ray + k) * 4 + 0..2]
// = the radiance of sample first_sample + k of probes[i] before the finite filter, [+3] = the stream's final counter;
// dirs[(i * samples_per_ray + k) * 4 + 0..2] = the unit direction drawn for it, [+3] = 0; basis[(i * samples_per_ray + k) * 9 + 0..8] =
// sh9 of that direction.  max_depth = 0: nothing is drawn, all three are zeros.  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_probe_err;

template <uint32_t F>
static void probes_run(const DScene &S, const GlobalMem &M, const RenderConsts &C, const vk_radiance_params *rp, const vk_ray *probes,
    uint64_t n, float *samples, float *dirs, float *basis) {
    for (uint64_t i = 0; i < n; i++) {
        const vk_ray &r = probes[i];
        for (uint32_t k = 0; k < rp->samples_per_ray; k++) {
            Rng g = radiance_rng(rp->seed, rp->first_index + i, rp->first_sample + k);
            V3 rgb = v3s(0.0f), u = v3s(0.0f);
            float Y[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (rp->max_depth != 0u) {
                Lane L;
                rgb = probe_sample<F, GlobalMem>(L, S, M, C, v3(r.origin[0], r.origin[1], r.origin[2]), r.time, r.tmax, g, u);
                g = L.rng;
                sh9(u, Y);
            }
            const uint64_t at = i * rp->samples_per_ray + k;
            float *o = samples + at * 4u;
            o[0] = rgb.x; o[1] = rgb.y; o[2] = rgb.z;
            memcpy(o + 3, &g.ctr, 4);
            if (dirs) { float *q = dirs + at * 4u; q[0] = u.x; q[1] = u.y; q[2] = u.z; q[3] = 0.0f; }
            if (basis) memcpy(basis + at * 9u, Y, sizeof(Y));
        }
    }
}

extern "C" {

const char *emu_probes_last_error() { return g_probe_err.c_str(); }

int emu_probes(const vk_scene_desc *desc, const vk_radiance_params *rp, const vk_ray *probes, uint64_t n, float *samples, float *dirs,
    float *basis, uint32_t *features_out) {
    if (!rp || (n != 0u && (!probes || !samples))) { g_probe_err = "null params, probes or samples"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_probe_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        if (features_out) *features_out = LS.features;
        with_radiance_features(LS.features, rp, [&](auto f) {
            probes_run<decltype(f)::value>(S, M, radiance_consts(rp), rp, probes, n, samples, dirs, basis);
        });
    });
}

}  // extern "C"
