// vk_emit.h — what the kernels of vk_kernels.h (vk_api.hip), of vk_adapt.hip and of vk_splat.hip share: the tile size, the fixed-point
// scale of the pixel sums with its conversions, and the start of a camera path of a film's window.  Device code, moved here from vk_kernels.h as it
// stood (vk_kernels.h defines non-template __global__ functions: one translation unit only may include it).  Everything is internal to
// the translation unit that includes it.
#ifndef VK_EMIT_H
#define VK_EMIT_H

#include <hip/hip_runtime.h>

#include "../../include/vecchio_amd.h"
#include "vk_trace.h"

using namespace vkd;

namespace {

constexpr int TILE = 8;   // 8x8 pixels = one wave

// the scale of the pixel sums (see vk_kernels.h "Pixel sums are ORDER-INDEPENDENT")
constexpr float ACCUM_SCALE = 67108864.0f;          // 2^26
// Components below 32 in magnitude — every sample of a scene without bright emitters, and nearly every one otherwise — fit 31 bits
// at 2^-26: ONE v_cvt_i32_f32 (truncating, like the 64-bit cast) and a sign extension, against ~17 instructions for the float ->
// 64-bit integer conversion the compiler has to expand.
constexpr float ACCUM_SMALL = 31.999f;
__device__ __forceinline__ long long to_fixed_small(float v) { return (long long)(int)(v * ACCUM_SCALE); }
__device__ __forceinline__ long long to_fixed(float v, float clampv) {
    v = fminf(fmaxf(v, -clampv), clampv);
    return (long long)(v * ACCUM_SCALE);             // scaling by a power of two is exact; the cast truncates toward zero
}

// A window of the film's frame and of its samples.  Its paths are numbered q = (row-major pixel of the window) * n_samples + k; path q is
// sample first_sample + k of that pixel.
struct EmitWindow {
    uint32_t x0, y0, win_width, first_sample, n_samples;
};
// The start of camera path q of window W, for one lane: start_sample_core itself — the render kernel's camera, on the film's frame —
// gives the ray, and the state resumes the sample's stream right behind the camera's draws.  The lens disk's rejection loop diverges, and
// may.  The ray (32 bytes), the state (48) and the id q are written at `slot` as vk_paths_begin would have staged them.
__device__ __forceinline__ void start_camera_path(const RenderConsts &C, const EmitWindow &W, uint32_t q, size_t slot, uint4 *rays,
                                                  uint4 *states, uint32_t *ids) {
    const uint32_t wp = q / W.n_samples, k = q - wp * W.n_samples;
    const uint32_t wy = wp / W.win_width, wx = wp - wy * W.win_width;
    Lane L;
    V3 o, d;
    float time;
    start_sample_core(L, C, W.x0 + wx, W.y0 + wy, W.first_sample + k, o, d, time);
    uint4 *r = rays + slot * 2u, *s = states + slot * 3u;
    r[0] = make_uint4(__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), 0x7F800000u /* tmax = +INFINITY */);
    r[1] = make_uint4(__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), __float_as_uint(time));
    s[0] = make_uint4(__float_as_uint(L.thr.x), __float_as_uint(L.thr.y), __float_as_uint(L.thr.z), L.depth);
    s[1] = make_uint4(__float_as_uint(L.acc.x), __float_as_uint(L.acc.y), __float_as_uint(L.acc.z), L.rng.ctr);
    s[2] = make_uint4((uint32_t)C.seed, (uint32_t)(C.seed >> 32), L.pixel, L.sample);
    ids[slot] = q;
}

}  // namespace

#endif
