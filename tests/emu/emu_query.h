// emu_query.h — TEST TOOL: what the four query emulators (emu_rays, emu_occlusion, emu_radiance, emu_irradiance) share: the scene on the
// tree view vk_api.hip aov_view promises (the tree as handed over; under VK_SCENE_FAST_ACCEL the rebuilt tree with its tie table) and the
// choice of F as the launchers make it.  Built into tests/emu's library only.
#ifndef EMU_QUERY_H
#define EMU_QUERY_H

#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/vecchio_amd_debug.h"
#include "../../vecchio_amd/csrc/vk_linearize.h"
#include "../../vecchio_amd/csrc/vk_trace.h"

using namespace vkd;

// linearises desc and calls fn(LS, S, M) with the tree view and its memory; a refusal's text goes to err
template <class Fn>
int with_query_scene(const vk_scene_desc *desc, std::string &err, Fn &&fn) {
    LinearScene LS;
    LinearizeOptions opt;
    opt.retree = (desc && (desc->flags & VK_SCENE_FAST_ACCEL)) ? 1 : 0;
    int st = linearize(desc, LS, err, opt);
    if (st != VK_OK) return st;
    DScene S = LS.host_view();
    if (!is_plain_tree_view(S)) {
        err = "the tree view came with a rebuilt form's gates"; return VK_ERR_BAD_ARG; }
    const GlobalMem M{S.items, S.spheres, S.sphere_mat, S.boxes};
    fn(LS, S, M);
    return VK_OK;
}

// fn(std::integral_constant<uint32_t, F>): a sphere-only world the fused sphere path, anything else the everything-variant; EXTRA: bits
// the tool adds (the radiance tools' VKF_INTEG_PDF)
template <uint32_t EXTRA = 0u, class Fn>
void with_features(uint32_t features, Fn &&fn) {
    if (features == 0u) fn(std::integral_constant<uint32_t, EXTRA>{});
    else fn(std::integral_constant<uint32_t, (uint32_t)VKF_ALL_SCENE | EXTRA>{});
}

// the radiance tools: the kernels' constants from the call's parameters, and the integrator's bit on F
inline RenderConsts radiance_consts(const vk_radiance_params *rp) {
    RenderConsts C;
    memset(&C, 0, sizeof(C));
    C.spp = rp->samples_per_ray; C.max_depth = rp->max_depth; C.seed = rp->seed;
    C.integrator = rp->integrator; C.background = rp->background;
    C.bg[0] = rp->background_color[0]; C.bg[1] = rp->background_color[1]; C.bg[2] = rp->background_color[2];
    return C;
}
template <class Fn>
void with_radiance_features(uint32_t features, const vk_radiance_params *rp, Fn &&fn) {
    if (rp->integrator == VK_INTEGRATOR_PDF) with_features<(uint32_t)VKF_INTEG_PDF>(features, fn);
    else with_features(features, fn);
}

#endif
