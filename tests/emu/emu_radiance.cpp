// emu_radiance.cpp — TEST TOOL: radiance queries (vk_trace_radiance) on the host: vk_trace.h radiance_sample on the tree view vk_api.hip
// aov_view promises (the tree as handed over; under VK_SCENE_FAST_ACCEL the rebuilt tree with its tie table), F chosen as the launcher
// chooses it.  samples[(i * samples_per_ray + k) * 4 + 0..2] = the radiance of sample first_sample + k of rays[i] before the finite
// filter, [+3] = the stream's final counter; keys as vk_debug_trace_radiance_samples takes them.  Built into tests/emu's library only.
#include "emu_query.h"

static thread_local std::string g_rad_err;

template <uint32_t F>
static void radiance_run(const DScene &S, const GlobalMem &M, const RenderConsts &C, const vk_radiance_params *rp, const vk_ray *rays,
    uint64_t n, const vk_debug_stream_key *keys, float *samples) {
    for (uint64_t i = 0; i < n; i++) {
        const vk_ray &r = rays[i];
        for (uint32_t k = 0; k < rp->samples_per_ray; k++) {
            Rng g;
            if (keys) { g = vk::rng_for_sample(keys[i].seed, keys[i].pixel, keys[i].sample + k); g.ctr = keys[i].ctr; }
            else g = radiance_rng(rp->seed, rp->first_index + i, rp->first_sample + k);
            V3 rgb = v3s(0.0f);
            if (rp->max_depth != 0u) {
                Lane L;
                rgb = radiance_sample<F, GlobalMem>(L, S, M, C, v3(r.origin[0], r.origin[1], r.origin[2]),
                                                    v3(r.direction[0], r.direction[1], r.direction[2]), r.time, r.tmax, g);
                g = L.rng;
            }
            float *o = samples + (i * rp->samples_per_ray + k) * 4u;
            o[0] = rgb.x; o[1] = rgb.y; o[2] = rgb.z;
            memcpy(o + 3, &g.ctr, 4);
        }
    }
}

extern "C" {

const char *emu_radiance_last_error() { return g_rad_err.c_str(); }

int emu_radiance(const vk_scene_desc *desc, const vk_radiance_params *rp, const vk_ray *rays, uint64_t n, const vk_debug_stream_key *keys,
    float *samples, uint32_t *features_out) {
    if (!rp || (n != 0u && (!rays || !samples))) { g_rad_err = "null params, rays or samples"; return VK_ERR_BAD_ARG; }
    return with_query_scene(desc, g_rad_err, [&](const LinearScene &LS, const DScene &S, const GlobalMem &M) {
        if (features_out) *features_out = LS.features;
        with_radiance_features(LS.features, rp, [&](auto f) {
            radiance_run<decltype(f)::value>(S, M, radiance_consts(rp), rp, rays, n, keys, samples);
        });
    });
}

}  // extern "C"
