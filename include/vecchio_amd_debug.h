/*
 * vecchio_amd_debug.h — test and diagnostic entry points.
 *
 * Not part of the drop-in boundary (include/vecchio_amd.h): nothing here replaces a reference
 * interface, and the Rust shim does not bind it.  Used by tests/ and bench.py only.
 * vk_debug_render_samples is in libvecchio_amd.so: it is vk_render with the PRODUCTION kernel's per-sample dump switched on.
 * vk_debug_phase_stats and vk_debug_math need kernels of their own (the instrumented STATS builds of the megakernel, the arithmetic
 * probe): they are in libvecchio_amd_debug.so, the same sources compiled with -DVK_DEBUG_LIB, so that the product library's code
 * object holds production kernels only.  A vk_scene belongs to the library that created it.
 */
#ifndef VECCHIO_AMD_DEBUG_H
#define VECCHIO_AMD_DEBUG_H

#include "vecchio_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* as vk_render, also returning every sample: samples_out[(pixel*spp + s)*4 + 0..2] = radiance
 * before the finite filter (main.rs:192), [+3] = the sample's u32 draw count (bit pattern) */
int vk_debug_render_samples(vk_scene *scene, const vk_camera *cam, const vk_render_params *params,
                            float *rgb_out, float *samples_out);
/* the render_kernel launches of a scene's last frame (host bookkeeping, tests): the role of each launch, the kernel instance
 * (the template key of render_kernel<F, LDS_SCENE, MINW, STATS, COST, GRID>) and its shape */
enum {
    VK_LAUNCH_MAIN = 0,          /* the frame's launch (single-launch shape) */
    VK_LAUNCH_DUAL_1024 = 1,     /* the dual launch of sphere-only scenes staged in LDS: its 1024-thread workgroups ... */
    VK_LAUNCH_DUAL_768 = 2,      /* ... and its 768-thread workgroups on the scene's second stream */
    VK_LAUNCH_PROBE = 3,         /* the probe launch of the dearest-first tile order (COST build) */
    VK_LAUNCH_REDO = 4,          /* exact re-treeing: the second launch, the queued samples on the tree as handed over */
    VK_LAUNCH_FALLBACK = 5       /* exact re-treeing: the fallback launch behind it (returns at once unless a queue overflowed) */
};
typedef struct vk_debug_launch {
    uint32_t role;               /* VK_LAUNCH_* */
    uint32_t features;           /* F */
    uint32_t lds_scene;          /* LDS_SCENE: the scene staged in LDS */
    uint32_t minw;               /* MINW: waves per SIMD of the build */
    uint32_t cost;               /* COST: the probe build */
    uint32_t grid_form;          /* GRID: the grid form of exact re-treeing */
    uint32_t grid_size;          /* workgroups */
    uint32_t block_size;         /* threads per workgroup */
    uint32_t shmem_bytes;        /* dynamic LDS bytes per workgroup */
} vk_debug_launch;
/* copies the first min(cap, *n) records of the last frame's launches into out (null when cap is 0); *n = how many there were.
 * A multi-device scene lists its parts' launches in part order. */
int vk_debug_last_launches(vk_scene *scene, vk_debug_launch *out, uint32_t cap, uint32_t *n);
/* a progressive handle's raw running fixed-point sums and error moments (width*height*3 each, y up, summed over the device parts):
 * what the adaptive judge reads.  Either may be NULL; m2 needs VK_PROGRESS_STDERR.  Waits for the last step. */
int vk_debug_progress_moments(vk_progress *pr, long long *run, double *m2);
/* Which form of the level kernel vk_denoise / vk_denoise_device launch on this scene from now on (vk_kernels.h): VK_DENOISE_FORM_AUTO
 * (the default) = per level the form that was measured faster; _PLAIN = one thread per pixel, every tap a global load, at every level;
 * _STAGED = the LDS-staged form at every level it exists for (tap spacing <= 32), plain beyond.  The results are bit-identical. */
enum { VK_DENOISE_FORM_AUTO = 0, VK_DENOISE_FORM_PLAIN = 1, VK_DENOISE_FORM_STAGED = 2 };
int vk_debug_denoise_form(vk_scene *scene, int form);
/* HIP-event times (ms) of the last vk_denoise on this scene: ms_out[0] the prepare kernel, ms_out[1 + i] level i (0 beyond `levels`) */
int vk_debug_denoise_last_ms(vk_scene *scene, double ms_out[9]);
/* render with the instrumented build of the sphere-only kernel and return the wave scheduler's
 * counters: [0] box steps (wave level) [1] lanes with box work summed over them [2] PRIM phases
 * [3] lanes with primitive work in them [4] SHADE+REFILL phases [5] lanes in them [6] rounds
 * [7] heavy-primitive phases; wave clocks spent in [8] BOX [9] light PRIM [10] heavy PRIM
 * [11] SHADE+REFILL phases, [12] total wave clocks, [13..15] SHADE split (material / refill / install), [16] the cooperative Perlin
 * turbulence ahead of the material code, [17] the cold-state load of the shading lanes; [18..23] reserved (0).
 * Sphere-only builds have no PRIM phases of their own (sphere tests run inside the box loop) and reuse four slots for the
 * box loop's exit tests: [2] exit tests, [7] live lanes, [9] lanes with a pending test, [10] lanes waiting for shading, each
 * summed over the exit tests.                                                                                   */
int vk_debug_phase_stats(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint64_t out[24]);
/* evaluate the shared host/device arithmetic ON THE DEVICE (host arrays in/out):
 * op 0 sin, 1 cos, 2 ln, 3 asin, 4 atan2(a,b), 5 pow5, 6 a/b, 7 sqrt(a), 8 draws, 9 a*b+a, 10 the sphere test's a/b,
 * 11 / 12 sincos .s / .c, 13 / 14 the samplers' sincos (0 <= a < 2^22) .s / .c                                      */
int vk_debug_math(int device, int op, const float *a, const float *b, float *out, size_t n);
/* libvecchio_amd_debug.so only: how many device resources the library's handles (scenes, progressive and temporal handles) own right
 * now: out[0] device buffers, [1] pinned host buffers, [2] events, [3] streams.  Back at its earlier value once a handle is destroyed. */
int vk_debug_live_objects(uint64_t out[4]);
/* vk_trace_occluded_device through a named form of occlusion_kernel (vk_kernels.h).  refill = 0: one ray per lane (the A/B partner of
 * the refill form; k and t are ignored).  refill != 0: the refill form with 64 * k rays per wave (k in 1..4096) that goes back to the
 * claim once t lanes are idle (t in 1..64).  The bytes are the same for every choice.  libvecchio_amd_debug.so holds both forms;
 * libvecchio_amd.so holds the form vk_trace_occluded launches and answers VK_ERR_UNSUPPORTED for the other one. */
int vk_debug_trace_occluded_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_occluded,
                                   void *hip_stream, int refill, uint32_t k, uint32_t t);
/* as vk_trace_radiance, returning every sample: samples_out[(i * samples_per_ray + k) * 4 + 0..2] = the radiance before the finite
 * filter, [+3] = the stream's counter at the sample's end (bit pattern); k = s - first_sample.  keys NULL: the public rule.  keys[i]
 * given: sample k of ray i uses rng_for_sample(keys[i].seed, keys[i].pixel, keys[i].sample + k) with its counter set to keys[i].ctr
 * before the first draw — a sample of vk_render is "the camera's draws, then ray_color on the same stream", so the query can resume
 * that stream right behind the camera's draws and be compared with the oracle sample by sample.  In both libraries. */
typedef struct vk_debug_stream_key { uint64_t seed; uint32_t pixel, sample, ctr, _pad; } vk_debug_stream_key;
int vk_debug_trace_radiance_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *rays, uint64_t n_rays,
                                    const vk_debug_stream_key *keys, float *samples_out, vk_stats *stats_out);
/* as vk_trace_irradiance, returning every sample: samples_out[(i * samples_per_ray + k) * 4 + 0..3] as above (the counter includes the
 * direction's two draws) and, with dirs_out given, dirs_out[(i * samples_per_ray + k) * 4 + 0..2] = the direction drawn for the sample,
 * [+3] = 0.  There are no keys: the public stream rule is the only one.  max_depth = 0: both are zeros.  In both libraries. */
int vk_debug_trace_irradiance_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *points, uint64_t n_points,
                                      float *samples_out /* n * spp * 4 */, float *dirs_out /* n * spp * 4, may be NULL */,
                                      vk_stats *stats_out);
/* as vk_trace_probes, returning every sample: samples_out[(i * samples_per_ray + k) * 4 + 0..2] = the radiance L before the finite
 * filter, [+3] = the stream's counter at the sample's end (it includes the direction's 3 * tries draws) and, with dirs_out given,
 * dirs_out[(i * samples_per_ray + k) * 4 + 0..2] = the unit direction u drawn for the sample, [+3] = 0.  There are no keys: the public
 * stream rule is the only one.  max_depth = 0: both are zeros.  In both libraries. */
int vk_debug_trace_probe_samples(vk_scene *scene, const vk_radiance_params *params, const vk_ray *probes, uint64_t n_probes,
                                 float *samples_out /* n * spp * 4 */, float *dirs_out /* n * spp * 4, may be NULL */,
                                 vk_stats *stats_out);
/* exactly the compaction a bounce of vk_paths_step runs (vk_kernels.h: count, scan, move), on host arrays staged once: items[n] and
 * ids[n] (each below n_ids) in; every output array is uploaded as the caller filled it, the three launches run, and every output array
 * is downloaded whole, so that what the kernels left alone comes back as it went in.  rays, states and ids_out hold n entries (the
 * survivors fill the first counts[VK_SHADE_SCATTERED] of them, in order), result_state and result_status n_ids entries (written at the
 * ids of the retired items only), counts[s] the items of status s (a status above 4 counts as 4).  n <= 2^24, n_ids <= 2^26; n == 0:
 * VK_OK, counts zeroed.  VK_ERR_BAD_ARG for a null pointer or an id >= n_ids.  Takes no stream.  In both libraries. */
int vk_debug_compact_paths(vk_scene *scene, const vk_shaded *items, const uint32_t *ids, uint64_t n, uint64_t n_ids, vk_ray *rays,
                           vk_path_state *states, uint32_t *ids_out, vk_path_state *result_state, uint32_t *result_status,
                           uint64_t counts[5]);
/* vk_debug_compact_paths with the termination rule *rp (vk_roulette_set's checks, in its words; NULL: VK_ERR_BAD_ARG) in the count
 * pass: roulette_count_kernel, then the scan and the move pass as they are.  The items are staged in a buffer of the hook's own: the
 * caller's array is not rewritten.  For driving the rule at its edge values and at exact sizes without a scene's paths.  Takes no stream.
 * In both libraries. */
int vk_debug_compact_roulette(vk_scene *scene, const vk_roulette_params *rp, const vk_shaded *items, const uint32_t *ids, uint64_t n,
                              uint64_t n_ids, vk_ray *rays, vk_path_state *states, uint32_t *ids_out, vk_path_state *result_state,
                              uint32_t *result_status, uint64_t counts[5]);
/* the device milliseconds of the handle's last bounce, part by part: ms[0] trace_paths_kernel, ms[1] shade_hits_kernel, ms[2] the
 * compaction's three launches (events vk_paths_step records between them; their sum is that bounce's share of kernel_ms).
 * VK_ERR_BAD_ARG for a null pointer or when no bounce has run since vk_paths_begin.  Takes no stream.  In both libraries. */
int vk_debug_paths_last_ms(vk_paths *p, double ms[3]);

/* a film's raw sums: width * height * 3 two's-complement 64-bit values in 2^-26 units, [(y * width + x) * 3 + c].  Waits.
 * VK_ERR_BAD_ARG for a null pointer.  Takes no stream.  In both libraries. */
int vk_debug_film_sums(vk_film *film, long long *sums);
/* the device milliseconds of the film's last vk_film_emit (ms[0]), vk_film_deposit (ms[1]) and vk_film_resolve (ms[2], the kernel without
 * the copy to the host), between two events around each; 0 for one that has not run.  Waits for those.  Takes no stream.  In both
 * libraries. */
int vk_debug_film_last_ms(vk_film *film, double ms[3]);
/* the form of film_deposit_kernel (vk_kernels.h) from the film's next vk_film_deposit on: PLAIN = three atomics per depositing lane; RUNS =
 * a wave's neighbouring lanes of one pixel summed first, the head lane of each run issuing the atomics.  Both give the same bytes.
 * VK_ERR_BAD_ARG for a null film or another form.  In both libraries. */
enum { VK_DEBUG_FILM_DEPOSIT_PLAIN = 0, VK_DEBUG_FILM_DEPOSIT_RUNS = 1 };
int vk_debug_film_deposit_form(vk_film *film, int form);

/* the device milliseconds of a regenerating batch's last bounce, part by part: ms[0] the top-up (regen_emit_kernel; next to nothing
 * where nothing was left to emit), ms[1] trace_paths_kernel, ms[2] shade_hits_kernel, ms[3] the compaction with the deposit (count, scan,
 * regen_move_kernel), from events vk_regen_step records between them on the handle; their sum is that bounce's share of kernel_ms.
 * VK_ERR_BAD_ARG for a null pointer, a batch that is not regenerating, or when no bounce has run since vk_regen_begin.  Takes no stream.
 * In both libraries. */
int vk_debug_regen_last_ms(vk_paths *batch, double ms[4]);

/* the error moments of a film with vk_adapt_enable, in vk_debug_progress_moments' layout: run = the sums at the last close (prev), m2 =
 * the batch-means moments, width * height * 3 values each, [(y * width + x) * 3 + c]; each may be NULL.  Waits.  VK_ERR_BAD_ARG for a
 * null film or one that is not enabled.  Takes no stream.  In both libraries. */
int vk_debug_adapt_moments(vk_film *film, long long *run, double *m2);
/* imposes a tile map on an enabled film and rebuilds the device list of active tiles from it: tile_n[t] (0 = active, else the count the
 * tile froze with) and tile_k[t] for every tile t = ty * tiles_x + tx.  The moments are left as they are.  For tests: the schedule of a
 * tile run on a chosen set of tiles.  VK_ERR_BAD_ARG for a null pointer or a film that is not enabled.  In both libraries. */
int vk_debug_adapt_set_tiles(vk_film *film, const uint32_t *tile_n, const uint32_t *tile_k);
/* the top-up kernel's own index code (vk_adapt.h adapt_locate) on the device, for paths first .. first + m of a tile run of n_samples over
 * the film's current tile set: pixel_out[i] = y * width + x and sample_out[i] = samples_done + k of path first + i.  m <= 2^24.
 * VK_ERR_BAD_ARG for a null pointer, a film that is not enabled, n_samples == 0 or first + m beyond the run's paths.  In both libraries. */
int vk_debug_adapt_sequence(vk_film *film, uint32_t n_samples, uint64_t first, uint32_t m, uint32_t *pixel_out, uint32_t *sample_out);

/* an accumulator's raw sums: width * height * 4 two's-complement 64-bit values in 2^-26 units, [(y * width + x) * 4 + c], c = r, g, b,
 * weight.  Waits.  VK_ERR_BAD_ARG for a null pointer.  Takes no stream.  In both libraries. */
int vk_debug_splat_sums(vk_splat *s, int64_t *sums4);
/* the form of splat_deposit_kernel (vk_splat.hip) from the accumulator's next vk_splat_deposit on: PLAIN = every (pixel, sum) a global
 * atomic; TILED = through an LDS tile per workgroup; DEFAULT = the measured one (DESIGN.md "Reconstruction filters").  All give the
 * same bytes.  VK_ERR_BAD_ARG for a null accumulator or another form.  In both libraries. */
enum { VK_DEBUG_SPLAT_FORM_DEFAULT = 0, VK_DEBUG_SPLAT_FORM_PLAIN = 1, VK_DEBUG_SPLAT_FORM_TILED = 2 };
int vk_debug_splat_form(vk_splat *s, uint32_t form);
/* the device milliseconds of the accumulator's last vk_splat_deposit (ms[0]: the kernel, without the copy of positions) and
 * vk_splat_resolve (ms[1]: the kernel without the copy to the host), between two events around each; 0 for one that has not run.
 * Waits for those.  Takes no stream.  In both libraries. */
int vk_debug_splat_last_ms(vk_splat *s, double ms[2]);

/* a robust accumulator's raw state: width * height * K * 4 two's-complement 64-bit values in the fixed logical order [(pixel * K + b) *
 * 4 + c], pixel = y * width + x, c = r, g, b (2^-26 units), count — whatever the device layout is.  Waits.  VK_ERR_BAD_ARG for a null
 * pointer.  Takes no stream.  In both libraries. */
int vk_debug_robust_sums(vk_robust *s, int64_t *out);
/* the device milliseconds of the accumulator's last vk_robust_deposit (ms[0]) and vk_robust_resolve (ms[1]: the kernel without the
 * copies to the host), between two events around each; 0 for one that has not run.  Waits for those.  Takes no stream.  In both
 * libraries. */
int vk_debug_robust_last_ms(vk_robust *s, double ms[2]);

/* a layer accumulator's raw state: width * height * n_layers * 4 two's-complement 64-bit values in the order [(pixel * n_layers + l) * 4
 * + c], pixel = y * width + x, c = r, g, b (2^-26 units), count.  Waits.  VK_ERR_BAD_ARG for a null pointer.  Takes no stream.  In both
 * libraries. */
int vk_debug_lpe_sums(vk_lpe *s, int64_t *out);
/* uploads sig[i] and term[i] as the tag of id i for the batch's started ids and binds the tracker to the batch as if it had recorded
 * every bounce the batch has run: the deposit can then be tested on injected results and tags.  vk_lpe_step's checks of the batch but
 * the binding's; null sig or term with started paths is VK_ERR_BAD_ARG.  Waits.  Takes no stream.  In both libraries. */
int vk_debug_lpe_set_tags(vk_lpe *s, vk_paths *batch, const uint32_t *sig, const uint32_t *term);
/* the device milliseconds of the tracker's last lpe_record_kernel launch (ms[0]), vk_lpe_deposit (ms[1]) and vk_lpe_resolve (ms[2]: the
 * kernel without the copies to the host), between two events around each; 0 for one that has not run.  Waits for those.  Takes no
 * stream.  In both libraries. */
int vk_debug_lpe_last_ms(vk_lpe *s, double ms[3]);

/* the histogram and the four counters (binned, below, above, nonfinite) of a tone handle's last vk_tone_meter, zeros before the first.
 * Waits.  VK_ERR_BAD_ARG for a null pointer.  Takes no stream.  In both libraries. */
int vk_debug_tone_histogram(vk_tone *t, uint32_t bins[640], uint64_t counters[4]);
/* the 510 thresholds H[1 .. 510] of VK_TONE_TRANSFER_SRGB or VK_TONE_TRANSFER_GAMMA22 as every handle holds them: host code, needs no
 * device.  VK_ERR_BAD_ARG for a null pointer or another transfer.  In both libraries. */
int vk_debug_tone_table(uint32_t transfer, float out[510]);
/* the form of vk_tone_meter's kernel from the next call on: LDS = a histogram per workgroup in LDS, flushed with one global atomic per
 * non-zero bin (the default, DESIGN.md "Display transform"); PLAIN = one global atomic per pixel.  Both give the same histogram.
 * VK_ERR_BAD_ARG for a null handle or another form.  In both libraries. */
enum { VK_TONE_FORM_LDS = 0, VK_TONE_FORM_PLAIN = 1 };
int vk_debug_tone_set_form(vk_tone *t, uint32_t form);
/* the device milliseconds of the handle's last meter kernel (ms[0]) and encode kernel (ms[1]: without the copy to the host), between
 * two events around each; 0 for one that has not run.  Waits for those.  Takes no stream.  In both libraries. */
int vk_debug_tone_last_ms(vk_tone *t, double ms[2]);

/* the form of vk_nlm_filter's kernel from the next call on: PLAIN = one lane per pixel, the definition straight from global memory;
 * TILED = a workgroup per tile, the frame staged in LDS and the patch sums shared between neighbouring pixels; AUTO (the default) = per
 * (search_radius, patch_radius) the one measured faster (DESIGN.md "Non-local means").  All give the same bits.  VK_ERR_BAD_ARG for a
 * null handle or another form.  In both libraries. */
enum { VK_NLM_FORM_AUTO = 0, VK_NLM_FORM_PLAIN = 1, VK_NLM_FORM_TILED = 2 };
int vk_debug_nlm_set_form(vk_nlm *h, uint32_t form);
/* the device milliseconds of the handle's last prepare kernel (ms[0]) and filter kernel (ms[1]: without copies), between two events
 * around each; 0 for one that has not run.  Waits for those.  Takes no stream.  In both libraries. */
int vk_debug_nlm_last_ms(vk_nlm *h, double ms[2]);

/* the form of vk_glare_apply's kernels from the next call on: PLAIN = one lane per output pixel straight from global memory, a launch
 * per down level, per up level and for the composite (2L - 2); FUSED = the down passes through LDS tiles, B_1 and B_2 in one launch,
 * and every level from the first that fits one workgroup's LDS in one tail launch; AUTO (the default) = per frame size and L the one
 * measured faster: PLAIN everywhere, FUSED won at no measured size (DESIGN.md "Glare").  All give the same bits.  VK_ERR_BAD_ARG for a null handle or another form.  In both libraries. */
enum { VK_GLARE_FORM_AUTO = 0, VK_GLARE_FORM_PLAIN = 1, VK_GLARE_FORM_FUSED = 2 };
int vk_debug_glare_set_form(vk_glare *g, uint32_t form);
/* the device milliseconds of the handle's last apply, between an event in front of its first kernel and one behind its last (without
 * copies); 0 before one.  Waits for it.  Takes no stream.  In both libraries. */
int vk_debug_glare_last_ms(vk_glare *g, double *ms);

/* the form of vk_upsample_apply's filter kernel from the next call on: PLAIN = one lane per high pixel, its taps' records straight from
 * global memory; TILED = a 256-lane workgroup stages the low footprint (at most 36 x 12 records) of its 32 x 8 high pixels in LDS and
 * filters from there; AUTO (the default) = a function of the two sizes alone, the form measured faster: TILED at every size (DESIGN.md
 * "Guided upsampling").  All give the same bits.
 * VK_ERR_BAD_ARG for a null handle or another form.  In both libraries. */
enum { VK_UPSAMPLE_FORM_AUTO = 0, VK_UPSAMPLE_FORM_PLAIN = 1, VK_UPSAMPLE_FORM_TILED = 2 };
int vk_debug_upsample_set_form(vk_upsample *u, uint32_t form);
/* the device milliseconds of the handle's last apply's filter kernel, between an event in front of it and one behind it (without copies
 * and without a prepare pass); 0 before one.  Waits for it.  Takes no stream.  In both libraries. */
int vk_debug_upsample_last_ms(vk_upsample *u, double *ms);

/* the library's twiddle table of a length N (vecchio_amd.h "Twiddle tables"): N / 2 entries of (re, im) into out[N].  VK_ERR_BAD_ARG for
 * a null pointer or an N that is no power of two in 2..4096.  Touches no device.  In both libraries. */
int vk_psf_debug_twiddles(uint32_t N, float *out);
/* one bare 2-D transform (vecchio_amd.h "2-D transform") of the caller's Px x Py complex values in host memory, (re, im) pairs, row y at
 * y * Px, in place: forward, or inverse with its closing multiplication by 1 / (Px * Py), by the kernels of the form VK_PSF_FORM_PLAIN
 * or VK_PSF_FORM_LDS on the scene's device.  VK_ERR_BAD_ARG for a null pointer, a size that is no power of two in 2..4096, inverse > 1,
 * another form.  Waits.  Takes no stream.  In both libraries. */
int vk_psf_debug_fft2(vk_scene *scene, uint32_t Px, uint32_t Py, uint32_t inverse, uint32_t form, float *data);
/* the device milliseconds of the four passes of the handle's last apply, between events recorded around them: rows forward (with the
 * bright part), columns forward, the product and rows inverse, columns inverse with the composite; zeros before an apply and after one
 * in the PLAIN form.  Waits for it.  Takes no stream.  In both libraries. */
int vk_psf_debug_last_pass_ms(vk_psf *h, double ms[4]);

/* the id of every sample vk_render_mattes would count, by the same per-lane code on the same lanes: ids_out[(y * width + x) * spp + k] is
 * the id of sample first_sample + k under `kind` (VK_MATTE_OBJECT or VK_MATTE_MATERIAL), spp = params->samples_per_pixel; pixels outside
 * the call's tile partition are left untouched.  vk_render_mattes' checks.  Waits.  In both libraries. */
int vk_debug_matte_samples(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                           uint32_t kind, uint32_t *ids_out);
#ifdef __cplusplus
}
#endif
#endif /* VECCHIO_AMD_DEBUG_H */
