// emu_irradiance.cpp — TEST TOOL: irradiance queries (vk_trace_irradiance) on the host: vk_trace.h irradiance_sample on the tree view
// vk_api.hip aov_view promises, F chosen as the launcher chooses it (as emu_radiance.cpp, which see).  samples[(i * samples_per_ray + k)
// * 4 + 0..2] = the radiance of sample first_sample + k of points[i] before the finite filter, [+3] = the stream's final counter;
// dirs[(i * samples_per_ray + k) * 4 + 0..2] = the direction drawn for it, [+3] = 0.  max_depth = 0: nothing is drawn, both are zeros.
// Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_irr_err;

template <uint32_t F>
static void irradiance_run(const DScene &S, const GlobalMem &M, const RenderConsts &C, const vk_radiance_params *rp, const vk_ray *points,
    uint64_t n, float *samples, float *dirs) {
    for (uint64_t i = 0; i < n; i++) {
        const vk_ray &r = points[i];
        for (uint32_t k = 0; k < rp->samples_per_ray; k++) {
            Rng g = radiance_rng(rp->seed, rp->first_index + i, rp->first_sample + k);
            V3 rgb = v3s(0.0f), d = v3s(0.0f);
            if (rp->max_depth != 0u) {
                Lane L;
                rgb = irradiance_sample<F, GlobalMem>(L, S, M, C, v3(r.origin[0], r.origin[1], r.origin[2]),
                                                      v3(r.direction[0], r.direction[1], r.direction[2]), r.time, r.tmax, g, d);
                g = L.rng;
            }
            float *o = samples + (i * rp->samples_per_ray + k) * 4u;
            o[0] = rgb.x; o[1] = rgb.y; o[2] = rgb.z;
            memcpy(o + 3, &g.ctr, 4);
            if (dirs) {
                float *q = dirs + (i * rp->samples_per_ray + k) * 4u;
                q[0] = d.x; q[1] = d.y; q[2] = d.z; q[3] = 0.0f;
            }
        }
    }
}

extern "C" {

const char *emu_irradiance_last_error() { return g_irr_err.c_str(); }

int emu_irradiance(const vk_scene_desc *desc, const vk_radiance_params *rp, const vk_ray *points, uint64_t n, float *samples, float *dirs,
    uint32_t *features_out) {
    if (!rp || (n != 0u && (!points || !samples))) { g_irr_err = "null params, points or samples"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_irr_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        if (features_out) *features_out = LS.features;
        with_radiance_features(LS.features, rp, [&](auto f) {
            irradiance_run<decltype(f)::value>(S, M, radiance_consts(rp), rp, points, n, samples, dirs);
        });
    });
}

}  // extern "C"
