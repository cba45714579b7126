/*
 * vecchio_amd.h — C ABI of the MI355X-native per-pixel sample loop.
 *
 * This is the drop-in boundary for ONE hot path of browserdotsys/vecchio: the closure at
 * reference src/main.rs:181-198 (pixel loop) and everything it calls (ray_color
 * main.rs:123-153, BVHNode::hit accel.rs:58-83, every Hittable::hit in hittable.rs, every
 * Material/Texture/PDF in material.rs / util.rs).  Everything above it (scene.rs builders,
 * BVHNode::new, the frame loop and the PPM writer of main.rs:155-221) stays on the host
 * side of this boundary.
 *
 * The reference has no FFI of its own (no extern "C" anywhere), so the entry points below
 * are "what a cgo/FFI binding for this path would bind": one scene upload
 * (vk_scene_create), one blocking call per camera frame (vk_render) placed where
 * main.rs:181-198 is today.  The Rust-side binding a maintainer would add is shown in
 * INTEGRATION.md and vecchio_amd/rust_shim/.
 *
 * Conventions
 *   - plain C, POD structs, caller owns every pointer it passes, library owns the handle.
 *   - every entry point returns an int status (VK_OK == 0); nothing unwinds across the
 *     boundary; vk_last_error() gives a thread-local message for the last failure.
 *   - the scene crosses the boundary as a *graph of tagged records* that mirrors the
 *     reference's trait objects 1:1 (one record per Arc<dyn Hittable/Material/Texture>),
 *     so that `flatten()` on the Rust side is a one-record push per object.  The library
 *     linearises that graph for the GPU itself (threaded pre-order BVH, SoA primitives).
 */
#ifndef VECCHIO_AMD_H
#define VECCHIO_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_ABI_VERSION 7   /* 7: progressive rendering (vk_progress_*; adaptive sampling added later as new symbols only, no struct changed: vk_progress_set_adaptive, vk_progress_tile_samples; vk_scene_desc unchanged: descriptions stamped 6 are accepted); 6: VK_SCENE_RCCL_GATHER, vk_scene_info.gather, vk_gather_backends; 5: rebuilt trees by default only where their exactness is proven; VK_SCENE_EMPIRICAL_TREES; vk_scene_info.tree */

/* ---- status codes (reference convention is panic!/unwrap, main.rs:166,202) ---------- */
enum {
    VK_OK = 0,
    VK_ERR_BAD_ARG = 1,      /* null pointer, bad index, time0>=time1 (main.rs:118 would panic) */
    VK_ERR_UNSUPPORTED = 2,  /* scene graph shape the device path does not implement      */
    VK_ERR_HIP = 3,          /* a HIP runtime call failed                                  */
    VK_ERR_NO_DEVICE = 4,    /* no gfx950 device / HIP runtime unusable                    */
    VK_ERR_OOM = 5
};

/* ---- object references -------------------------------------------------------------
 * A vk_ref names one Arc<dyn Hittable>: kind in bits 31..28, FlipFace parity in bit 27
 * (FlipFace, hittable.rs:294-312, only negates `front`, so wrapping is an XOR of this
 * bit), index into the per-kind array in bits 26..0.                                    */
typedef uint32_t vk_ref;
enum {
    VK_KIND_NONE = 0,
    VK_KIND_BVH = 1,           /* accel.rs:52-56                 */
    VK_KIND_SPHERE = 2,        /* hittable.rs:46-51              */
    VK_KIND_MOVING_SPHERE = 3, /* hittable.rs:136-144            */
    VK_KIND_RECT = 4,          /* hittable.rs:199-210            */
    VK_KIND_LIST = 5,          /* Vec<Arc<HittableSS>>, hittable.rs:380 (Boxy::sides) */
    VK_KIND_MEDIUM = 6,        /* hittable.rs:436-440            */
    VK_KIND_TRANSLATE = 7,     /* hittable.rs:500-504            */
    VK_KIND_ROTATE = 8         /* hittable.rs:534-539,631,720    */
};
#define VK_REF_FLIP 0x08000000u
#define VK_REF_INDEX_MASK 0x07FFFFFFu
#define VK_MAKE_REF(kind, index) ((((uint32_t)(kind)) << 28) | ((uint32_t)(index) & VK_REF_INDEX_MASK))
#define VK_REF_KIND(r) ((r) >> 28)
#define VK_REF_INDEX(r) ((r) & VK_REF_INDEX_MASK)

/* ---- hittables ---------------------------------------------------------------------- */
typedef struct vk_bvh_node {   /* accel.rs:52-56 — 32 bytes, the canonical node record */
    float bb_min[3];
    float bb_max[3];
    vk_ref left;
    vk_ref right;
} vk_bvh_node;

typedef struct vk_sphere {     /* hittable.rs:47-51; radius may be negative (scene.rs:123-127) */
    float center[3];
    float radius;
    uint32_t material;
} vk_sphere;

typedef struct vk_moving_sphere { /* hittable.rs:137-144 */
    float center0[3];
    float center1[3];
    float time0, time1;
    float radius;
    uint32_t material;
} vk_moving_sphere;

typedef struct vk_rect {       /* hittable.rs:200-210; XY=(0,1,2) XZ=(0,2,1) YZ=(1,2,0) */
    float c0, c1, d0, d1, k;
    uint8_t axis0, axis1, axis2, _pad;
    uint32_t material;
} vk_rect;

typedef struct vk_list {       /* Vec<Arc<HittableSS>>: items[first .. first+count) */
    uint32_t first;
    uint32_t count;
} vk_list;

typedef struct vk_medium {     /* hittable.rs:436-440; material = the Isotropic phase function */
    vk_ref boundary;
    float neg_inv_density;
    uint32_t material;
} vk_medium;

typedef struct vk_translate {  /* hittable.rs:500-504 */
    vk_ref child;
    float offset[3];
} vk_translate;

typedef struct vk_rotate {     /* hittable.rs:534-539 (Y), 631-636 (X), 720-725 (Z) */
    vk_ref child;
    uint32_t axis;             /* 0 = RotateX, 1 = RotateY, 2 = RotateZ */
    float sin_theta, cos_theta;
} vk_rotate;

/* ---- materials (material.rs) -------------------------------------------------------- */
enum {
    VK_MAT_LAMBERTIAN = 0,   /* material.rs:45-109   texture */
    VK_MAT_METAL = 1,        /* material.rs:111-142  texture, param = fuzz */
    VK_MAT_DIELECTRIC = 2,   /* material.rs:144-207  param = ref_idx */
    VK_MAT_DIFFUSE_LIGHT = 3,/* material.rs:209-226  texture = emit */
    VK_MAT_ISOTROPIC = 4,    /* material.rs:436-465  texture */
    VK_MAT_SPEC_DIFFUSE = 5  /* material.rs:467-488  a = specular material, b = diffuse material, param = pct */
};
/* A SpecDiffuse may have any material as a child, another SpecDiffuse included (Arc<MaterialSS>).  The device resolves at most
 * VK_MAX_SPEC_DIFFUSE_DEPTH SpecDiffuses on a path from a material to a leaf, counted along the deeper of the two children (the draw
 * loop and the scattering_pdf loop of shade_core and the stack of aov_albedo, vk_trace.h, hold that many).  Scene creation returns
 * VK_ERR_UNSUPPORTED, with the limit in the message, for a deeper acyclic graph, and VK_ERR_BAD_ARG ("cyclic") for a SpecDiffuse that
 * reaches itself through a or b. */
#define VK_MAX_SPEC_DIFFUSE_DEPTH 8u
typedef struct vk_material {
    uint32_t kind;
    uint32_t texture;
    float param;
    uint32_t a, b;
} vk_material;

enum {
    VK_TEX_SOLID = 0,   /* material.rs:233-242 color            */
    VK_TEX_CHECKER = 1, /* material.rs:244-259 a = odd, b = even (texture indices) */
    VK_TEX_IMAGE = 2,   /* material.rs:261-304 a = image index  */
    VK_TEX_NOISE = 3    /* material.rs:416-434 a = perlin index, scale */
};
/* A checker may have any texture as a child, another checker included (Arc<TextureSS>).  The device resolves at most
 * VK_MAX_CHECKER_DEPTH checkers on a path from a texture to a leaf, counted along the deeper of the two children (texture_value,
 * vk_trace.h, walks 16 records: 15 checkers and the leaf).  Scene creation returns VK_ERR_UNSUPPORTED, with the limit in the message,
 * for a deeper acyclic graph, and VK_ERR_BAD_ARG ("cyclic") for a checker that reaches itself through a or b. */
#define VK_MAX_CHECKER_DEPTH 15u
typedef struct vk_texture {
    uint32_t kind;
    float color[3];
    uint32_t a, b;
    float scale;
} vk_texture;

typedef struct vk_image {      /* decoded 8-bit RGB, row 0 = top (material.rs:261-279) */
    uint32_t width, height;
    const uint8_t *rgb;        /* width*height*3 bytes */
} vk_image;

typedef struct vk_perlin {     /* material.rs:306-311 */
    float ranvec[256][3];
    uint32_t perm_x[256], perm_y[256], perm_z[256];
} vk_perlin;

/* ---- the flattened scene ------------------------------------------------------------ */
/* An array pointer that is NULL while its count is not 0 is refused with VK_ERR_BAD_ARG (each record array and lights). */
typedef struct vk_scene_desc {
    uint32_t abi_version;      /* VK_ABI_VERSION (6 is accepted too: the description has not changed since) */
    uint32_t n_bvh;            const vk_bvh_node *bvh;
    uint32_t n_spheres;        const vk_sphere *spheres;
    uint32_t n_moving_spheres; const vk_moving_sphere *moving_spheres;
    uint32_t n_rects;          const vk_rect *rects;
    uint32_t n_lists;          const vk_list *lists;
    uint32_t n_list_items;     const vk_ref *list_items;
    uint32_t n_media;          const vk_medium *media;
    uint32_t n_translates;     const vk_translate *translates;
    uint32_t n_rotates;        const vk_rotate *rotates;
    uint32_t n_materials;      const vk_material *materials;
    uint32_t n_textures;       const vk_texture *textures;
    uint32_t n_images;         const vk_image *images;
    uint32_t n_perlins;        const vk_perlin *perlins;
    vk_ref world;              /* main.rs:168 world_bvh */
    uint32_t n_lights;         const vk_ref *lights;  /* main.rs:169 config.lights */
    uint32_t flags;            /* VK_SCENE_* (ABI 2); 0 = results of the tree handed over (see below) */
} vk_scene_desc;

/* vk_scene_desc.flags.
 * 0 (default): every result is the one BVHNode::hit (accel.rs:58-83) gives on the tree handed over.  The library walks that tree,
 * with one exception: a world of spheres only may be walked on a tree REBUILT over the reference's leaf units, "exact re-treeing"
 * (DESIGN.md section 5).  Every object stays gated by the box the reference gates it with, grown by a bound on how far off its sphere
 * an f32 Sphere::hit (hittable.rs:65-95) can report a hit; the rebuilt walk then finds every hit the reference's walk can accept,
 * and whenever its winner is not certain to be the reference's too — a hit not safely behind its own box's entry, a ray from outside
 * the region the bound was derived for — the tree as handed over decides (the segment is walked again, or its sample is rendered by
 * a second launch).  That this reproduces BVHNode::hit is a THEOREM given the bound (the "gate lemma"; forward error analysis, K < 30
 * against the 32 used; tests/test_gate_lemma.py attacks it with 10^7 adversarial rays).  Three proven forms (vk_scene_info.tree).  The
 * NEAR form (ABI 6, VK_TREE_REBUILT_NEAR): every sphere behind its OWN box, which is sound for ray origins within a trusted radius of
 * the sphere (~144 radii); a segment's result is taken only if its hit lies within that reach of its origin or the ray provably runs
 * clear of every small sphere beyond it, and every other segment is decided by the tree as handed over (both trees stay in device
 * memory; docs/gate_lemma.md section 7).  It is the default where its reach spans the world's small spheres
 * and where the other form is too dear (BVHNode::new's long leaf boxes on the 1 M-sphere
 * stress scene: +85 %).  The UNIT form (VK_TREE_REBUILT_PROVEN): the reference's leaf units as gates, grown by the bound — where that is
 * cheap and the near form's reach does not span the world.  And, where the world's small spheres lie in a layer across y and the scene
 * is staged in LDS (the InOneWeekend scene), no tree at all — the GRID form (VK_TREE_REBUILT_GRID): every sphere that can hold a
 * candidate for the ray is found through a grid over the layer and tested, the winner checked like the other forms' (docs/gate_lemma.md
 * section 8; +33 % throughput over the tree handed over).  A world for which no form applies is walked as handed over.
 * VK_SCENE_REFERENCE_TREE: walk the tree handed over and nothing else.
 * VK_SCENE_EMPIRICAL_TREES: allow the rebuilt tree also where NEITHER proven form applies (since ABI 6: worlds with a sphere far
 * smaller than the rest; the environment's VK_GATE_PROOF=0 prefers it to the proven forms, for comparisons) — with the units' boxes as
 * handed over and the closest hit so far padded by 1/16 instead.  NOT proven: a hit that precedes its unit's box entry by more than 1/16 and,
 * in the reference's visiting order only, wins against a hit inside that gap is missed.  It takes a ray that grazes a sphere where the
 * sphere touches its box, within ~1e-5 of parallel to that face of a long box; tests/test_gate_lemma.py constructs one and shows the
 * wrong result.  Measured on natural frames: 0 differing pixels in 12.6 G samples (40 worlds, profiles/r03/exact_retree_seeds.log);
 * the 1 M-sphere stress scene runs 1.7x faster than on the tree handed over.
 * VK_SCENE_FAST_ACCEL: the library may rebuild the acceleration structure over subtrees whose objects are all
 * Sphere / Rect / Boxy / lists of those (no ConstantMedium, no transform, no negative-radius sphere), object by object:
 * BVHNode::hit's result does not depend on the tree over such objects in exact arithmetic, and exact ties in t are resolved as the
 * reference resolves them.  What it cannot reproduce is floating-point noise: an f32 Sphere::hit that reports a hit OUTSIDE the
 * sphere's own bounding box is found or not depending on which enclosing boxes a tree happens to have — in the reference as much
 * as here, whose own tree is random (accel.rs:99-100).  Measured: the InOneWeekend scene's full 1920x1080x1024-spp frame is
 * bit-identical with and without the flag; on the 1 M-sphere stress scene 0.19 % of the samples differ — as many as between two
 * reference-style trees over the same world (profiles/r03/tree_variation.log).  Does not match a seeded reference run sample for
 * sample.
 * VK_SCENE_RCCL_GATHER (ABI 6; vk_scene_create_multi only, no effect on a pixel): the tile slabs travel to devices[0] by RCCL — one
 * communicator per device (ncclCommInitAll), one grouped ncclSend / ncclRecv pair per device and frame, on the devices' own streams —
 * instead of hipMemcpyPeerAsync.  librccl.so is loaded when the flag is first used, never linked; if it cannot be loaded, or a device
 * is listed twice (one communicator rank per device), the scene falls back to peer copies and says so on stderr
 * (vk_scene_info.gather tells which). */
enum { VK_SCENE_FAST_ACCEL = 1, VK_SCENE_REFERENCE_TREE = 2, VK_SCENE_EMPIRICAL_TREES = 4, VK_SCENE_RCCL_GATHER = 8 };

/* ---- camera: the ten fields of main.rs:57-68, computed by Camera::new on the host --- */
typedef struct vk_camera {
    float origin[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
    float u[3], v[3], w[3];
    float lens_radius;
    float time0, time1;
} vk_camera;

/* ---- render parameters: the reference's compile-time constants, made arguments ------ */
enum {
    VK_INTEGRATOR_PDF = 0,     /* HEAD ray_color, main.rs:123-153 (scatter_with_pdf + mixture PDF) */
    VK_INTEGRATOR_SCATTER = 1  /* InOneWeekend/TheNextWeek tags: emitted + attenuation*L via
                                  Material::scatter (material.rs:21-28,85-90,118-132,150-175,442-446) */
};
enum {
    VK_BACKGROUND_SOLID = 0,   /* main.rs:124 (HEAD: black) */
    VK_BACKGROUND_SKY = 1      /* InOneWeekend gradient (1-t)*white + t*(0.5,0.7,1.0), t = 0.5*(unit(d).y+1) */
};
typedef struct vk_render_params {
    uint32_t width, height;        /* main.rs:171-172 */
    uint32_t samples_per_pixel;    /* main.rs:28 */
    uint32_t max_depth;            /* main.rs:29; depth starts at 1, path stops when depth > max_depth */
    uint64_t seed;                 /* replaces rand::thread_rng(): counter-based, keyed (seed,pixel,sample) */
    uint32_t integrator;           /* VK_INTEGRATOR_* */
    uint32_t background;           /* VK_BACKGROUND_* */
    float background_color[3];     /* for VK_BACKGROUND_SOLID */
    /* pixel-tile partition for multi-GPU: 8x8-pixel tiles are dealt round-robin; this call
     * renders tiles t with t % tile_world == tile_rank.  (0,1) or (0,0) = whole image. */
    uint32_t tile_rank, tile_world;
    /* what vk_render / vk_render_device write (ABI 2): VK_OUTPUT_F32 = the pixel means as above;
     * VK_OUTPUT_RGB8 = the reference's output stage fused behind the render: Vec3::to_color
     * (vec3.rs:54-61) per pixel and the PPM writer's top-down row order (main.rs:209) —
     * width*height*3 BYTES, row 0 = TOP.  A multi-GPU host gathers these (4x less xGMI traffic). */
    uint32_t output_format;
} vk_render_params;
enum { VK_OUTPUT_F32 = 0, VK_OUTPUT_RGB8 = 1 };

typedef struct vk_stats {
    uint64_t samples;          /* pixel-samples rendered by this call            */
    double seconds;            /* wall seconds of the call (incl. gather/copies) */
    double kernel_ms;          /* HIP-event time of the megakernel launch(es)    */
    uint32_t kernel_launches;
    uint32_t scene_in_lds;     /* 1 if the linear BVH + primitives were LDS-resident */
    /* ABI 3.  Pixel sums (`c += color`, main.rs:193) are kept as 64-bit fixed point with 2^-26 resolution so that they do not
     * depend on the order samples finish in: a sample component below 2^-26 (1.5e-8) adds 0, and a component beyond
     * +-min(1e10, 1.3e11 / samples_per_pixel) is CLAMPED to that (the sums saturate, they never wrap).  The reference adds such
     * a sample in f32; this counts the samples of the call that were clamped (0 on every BASELINE config): non-zero means the
     * frame's brightest pixels deviate from the reference's.  vk_render fills it; after vk_render_device use
     * vk_scene_last_clamped_samples().                                                                                     */
    uint64_t clamped_samples;
} vk_stats;

typedef struct vk_scene vk_scene;  /* opaque */

/* replaces: nothing (version handshake for the Rust shim) */
int vk_abi_version(void);
/* replaces: nothing (reference is single-device CPU); number of usable gfx950 devices */
int vk_device_count(void);
/* replaces: panic!/unwrap messages (main.rs:166,202); thread-local, never NULL */
const char *vk_last_error(void);
/* how a multi-device scene can move its tile slabs: bit 0 = peer copies (always), bit 1 = RCCL (librccl.so loads and exports what
 * VK_SCENE_RCCL_GATHER needs).  Touches no device.  replaces: nothing */
int vk_gather_backends(void);

/* replaces: the ownership hand-off at main.rs:168-169 (Arc::new(BVHNode::new(..)),
 * Arc::new(config.lights)): deep-copies the described graph, linearises it and uploads it
 * to `device`.  The scene DESCRIPTION is immutable afterwards and may be rendered many times
 * (RotatingCamera, scene.rs:65-91).  The handle also owns per-launch scratch (work counter,
 * chunk partials, tile order): AT MOST ONE render may be in flight per vk_scene — calls on one
 * scene must be made from one thread at a time and be stream-ordered (the reference's frame loop,
 * main.rs:176, is exactly that); concurrent frames need one vk_scene each.
 * STREAM-ORDERED, for the entry points that take a `hip_stream` (the *_device calls), means two things:
 *   - Successive *_device calls on one scene (and on its vk_progress / vk_temporal handles) are ordered by the caller's stream(s): a
 *     call's work starts after everything enqueued on its hip_stream before the call, and whatever is enqueued on that stream once the
 *     call has returned starts after that work; the library's own streams fork from and join back into hip_stream.  Calls on ONE stream
 *     need nothing else; a caller that moves to another stream orders the two itself (an event), as for any work on its buffers.
 *   - Arguments passed by pointer to host structs (camera, render / guide / trace / denoise params) are consumed before the call
 *     returns: the caller may overwrite or free them at once.  Device buffers are read and written in stream order.
 * What is NOT promised: a blocking host-pointer call (vk_render, vk_progress_step, vk_render_aov, vk_trace_rays, vk_denoise,
 * vk_temporal_accumulate, ...) works on the NULL stream and does not wait for a *_device call still in flight on the same scene.  The
 * NULL stream waits for blocking streams only: after *_device calls on a non-blocking stream (hipStreamNonBlocking; PyTorch's streams
 * are) the caller synchronises that stream before the blocking call.  The calls documented as waiting (vk_scene_last_*,
 * vk_progress_get_info, vk_progress_stderr_device, vk_temporal_get_info, ...) wait for the scene's or the handle's last enqueued work.
 * tests/test_gpu_stream_order.py holds every *_device entry point to the two promises on a non-blocking stream of the caller's.      */
int vk_scene_create(const vk_scene_desc *desc, int device, vk_scene **out);
/* same, uploaded to EVERY device in devices[0..n_devices) ("uploads to every participating
 * GPU").  vk_render / vk_render_device on such a scene deal this call's 8x8 tiles round-robin over the
 * devices, render each share on that device's own stream, move the tile slabs to devices[0] with peer
 * copies over xGMI — or, with VK_SCENE_RCCL_GATHER, with RCCL send / receive pairs — (one message per device: the path's only
 * exchange), de-interleave them
 * on devices[0] and, for vk_render, do ONE device-to-host copy.  The image is bit-identical to the
 * one-device image.  A device may be listed more than once (shares run concurrently on it).       */
int vk_scene_create_multi(const vk_scene_desc *desc, const int *devices, int n_devices, vk_scene **out);
void vk_scene_destroy(vk_scene *scene);

/* replaces: the closure body at main.rs:181-198 for one Camera yielded by cam_iter
 * (main.rs:176).  Blocking.  rgb_out is caller-owned, width*height*3 floats, index
 * (y*width + x)*3 with y = 0 the BOTTOM row (main.rs:182-183,209) — or, with
 * params->output_format == VK_OUTPUT_RGB8, width*height*3 bytes, top row first.  Pixels outside
 * this call's tile partition are left untouched.  max_depth == 0 renders the reference's result
 * for MAX_DEPTH = 0: every sample is (0,0,0) (main.rs:126-128).                            */
int vk_render(vk_scene *scene, const vk_camera *cam, const vk_render_params *params,
              float *rgb_out, vk_stats *stats_out);

/* same as vk_render but the framebuffer is a device pointer on the scene's device and the
 * work is enqueued on `hip_stream` (a hipStream_t, or NULL for the default stream) without
 * a host synchronisation; used by the multi-GPU host (one process per GPU) so the RCCL
 * gather can be enqueued behind it.  stats_out->kernel_ms is not filled.  For a multi-device
 * scene the pointer and the stream belong to devices[0].                                 */
int vk_render_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params,
                     void *d_rgb_out, void *hip_stream, vk_stats *stats_out);

/* replaces: Vec3::to_color (vec3.rs:54-61) applied per pixel at main.rs:211 — sqrt gamma,
 * clamp to [0,0.999], *256, truncate — plus the top-down row order of main.rs:209.
 * d_rgb: width*height*3 floats (y up); d_rgb8_out: width*height*3 bytes, row 0 = TOP.  */
int vk_to_color_device(vk_scene *scene, const void *d_rgb, uint32_t width, uint32_t height,
                       void *d_rgb8_out, void *hip_stream);

/* ---- tile slabs: the exchange format of the multi-GPU host.  Rank r of w renders the 8x8 tiles t = r, r + w, r + 2w ...
 * (vk_render_params.tile_rank / tile_world); its SLAB is those tiles packed one after the other, 64 pixel slots per tile (slot
 * (y % 8) * 8 + x % 8; slots outside the image are present and unused), 3 components per slot: floats (VK_OUTPUT_F32) or bytes through
 * Vec3::to_color (VK_OUTPUT_RGB8, vec3.rs:54-61: a quarter of the traffic).  A one-process-per-GPU host calls vk_render_device
 * (VK_OUTPUT_F32) and vk_pack_tiles_device on every rank, gathers the equal-sized slabs on rank 0 (RCCL: ONE message per GPU, the
 * path's only exchange) and calls vk_unpack_tiles_device once per rank there.  replaces: nothing (single address space, main.rs:181). */
/* bytes of one rank's slab; the largest over the ranks (they differ by at most one tile) when tile_rank >= tile_world */
size_t vk_tile_slab_bytes(uint32_t width, uint32_t height, uint32_t output_format, uint32_t tile_rank, uint32_t tile_world);
/* d_fb: this rank's f32 framebuffer (width*height*3 floats, y up) on the scene's device -> d_slab */
int vk_pack_tiles_device(vk_scene *scene, const void *d_fb, uint32_t width, uint32_t height, uint32_t output_format,
                         uint32_t tile_rank, uint32_t tile_world, void *d_slab, void *hip_stream);
/* d_slab of rank tile_rank -> its tiles of the full image d_img on the scene's device: f32, y up (VK_OUTPUT_F32), or bytes, top row
 * first (VK_OUTPUT_RGB8, main.rs:209) */
int vk_unpack_tiles_device(vk_scene *scene, const void *d_slab, uint32_t width, uint32_t height, uint32_t output_format,
                           uint32_t tile_rank, uint32_t tile_world, void *d_img, void *hip_stream);

/* introspection used by bench/tests: bytes of the linearised scene, item counts */
typedef struct vk_scene_info {
    uint32_t n_items;          /* 32-byte linear BVH records */
    uint32_t n_prims;          /* primitive records */
    uint32_t n_instances;
    uint64_t device_bytes;
    uint32_t lds_bytes;        /* bytes staged into LDS per workgroup (0 = not resident) */
    uint32_t features;         /* VKF_* mask of the kernel variant selected */
    uint32_t tree;             /* VK_TREE_*: what the world is walked on (ABI 5; see vk_scene_desc.flags) */
    /* frames for which a rebuilt tree is suspended (the tree as handed over is walked meanwhile): a frame that sends more than a quarter
     * of its samples to the tree as handed over anyway, or more than the queues between the two launches hold, pauses the rebuilt tree
     * for 32 frames, twice as long at every relapse; 0 = in use.  As of the last frame whose end the library has seen. */
    uint32_t tree_suspended_frames;
    uint32_t gather;           /* VK_GATHER_*: how a multi-device scene moves its tile slabs to devices[0] (ABI 6) */
} vk_scene_info;
enum { VK_GATHER_NONE = 0 /* one device */, VK_GATHER_PEER_COPY = 1 /* hipMemcpyPeerAsync over xGMI */, VK_GATHER_RCCL = 2 };
enum {
    VK_TREE_HANDED_OVER = 0,        /* the tree of the description, item for item */
    VK_TREE_REBUILT_PROVEN = 1,     /* exact re-treeing with grown gates: results proven to be the handed-over tree's */
    VK_TREE_REBUILT_EMPIRICAL = 2,  /* exact re-treeing without them (VK_SCENE_EMPIRICAL_TREES): measured, not proven */
    VK_TREE_REBUILT_FAST = 3,       /* VK_SCENE_FAST_ACCEL */
    VK_TREE_REBUILT_NEAR = 4,       /* exact re-treeing, near form (ABI 6): every sphere behind its own box, a segment's result taken only
                                       where no sphere beyond that box's trusted radius can matter, else walked again on the tree handed
                                       over: proven like VK_TREE_REBUILT_PROVEN; taken first where its reach spans the world's small
                                       spheres, and for worlds whose leaf units are too long for the unit form */
    VK_TREE_REBUILT_GRID = 5        /* exact re-treeing, grid form (ABI 6, round 5): no tree at all — a world of spheres whose small spheres
                                       lie in a layer across y is walked on a uniform grid over the layer; every sphere that can hold a
                                       candidate for the ray is tested, the winner is checked like the other forms' and the tree handed
                                       over decides where that fails: proven like them (docs/gate_lemma.md section 8) */
};
int vk_scene_get_info(const vk_scene *scene, vk_scene_info *out);

/* One part of a scene — a multi-device scene has one per entry of devices[], an ordinary scene one — for a host that wants to SAY what
 * ran where (bench.py --in-library): the device's index, name and PCI bus id, whether it can address devices[0]'s memory (if not, its
 * tile slab travels through host memory), and the HIP-event time of the part's launches in the last frame (waits for them; -1 before
 * the first frame).  replaces: nothing (ABI 6) */
typedef struct vk_part_info {
    uint32_t n_parts;
    int32_t device;
    char name[64];
    char pci_bus_id[32];
    uint32_t can_access_landing_device;
    double kernel_ms;
} vk_part_info;
int vk_scene_part_info(vk_scene *scene, int part, vk_part_info *out);

/* HIP-event time (ms) of the launches enqueued by the last vk_render / vk_render_device on
 * this scene, on the stream they were launched on; waits for their end event.  (For a
 * multi-device scene: the slowest device's time.)                                         */
int vk_scene_last_kernel_ms(vk_scene *scene, double *ms_out);

/* see vk_stats.clamped_samples; waits for the end of the last render enqueued on this scene */
int vk_scene_last_clamped_samples(vk_scene *scene, uint64_t *count_out);
/* Exact re-treeing (see vk_scene_desc.flags): samples of the last render that were rendered by the second launch, on the tree as
 * handed over; waits for the render's end. */
int vk_scene_last_requeued_samples(vk_scene *scene, uint64_t *count_out);

/* ---- progressive rendering (ABI 7) ---------------------------------------------------
 * replaces: nothing (the reference renders each frame in one go, main.rs:181-198).  A vk_progress accumulates ONE frame — one camera, one
 * vk_render_params — over successive sample WINDOWS: a preview after every step, a stop when the image is good enough, a time budget
 * spent in slices, short launches on a shared card.  params->samples_per_pixel at create is the frame's BUDGET: the steps together may
 * render at most that many samples per pixel.
 *
 * Bit-identity.  Every sample is keyed by its index (RNG keyed by (seed, pixel, sample)) and pixel sums are exact 64-bit fixed point, so
 * a step renders samples [samples_done, samples_done + n) of every pixel of the partition and adds them into running sums that live in
 * the handle (one set per device of the scene).  After any sequence of steps the image written is, bit for bit, the image vk_render
 * gives with the same params at samples_per_pixel = samples_done — as long as no sample was clamped (vk_progress_info.clamped_samples
 * == 0): the clamp (see vk_stats.clamped_samples) is the one of the BUDGET's one-shot frame, so the final image of a frame rendered to
 * its budget is vk_render's image of the budget exactly, clamped samples or not.
 *
 * Calls.  A step writes the running mean as vk_render / vk_render_device write theirs: f32 with y up, or with params->output_format ==
 * VK_OUTPUT_RGB8 bytes with the top row first; only this partition's tiles are written.  n_samples == 0, samples_done + n_samples >
 * budget, a null handle and the argument checks of vk_render each return VK_ERR_BAD_ARG, enqueue nothing and leave the handle as it was.
 * The rule "at most one render in flight per vk_scene" covers vk_render and progress steps together: they may be interleaved on one
 * scene (stream-ordered), the running sums belong to the handle.  Destroy the handle before its scene.                           */
typedef struct vk_progress vk_progress;   /* opaque */
enum { VK_PROGRESS_STDERR = 1 };          /* also keep the error moments (24 more bytes per pixel and device) */
typedef struct vk_progress_info {
    uint32_t samples_done;     /* samples 0 .. samples_done-1 of every pixel of the partition are in the sums */
    uint32_t samples_budget;   /* params->samples_per_pixel at create: the frame's total, fixes the clamp */
    uint32_t steps;            /* windows since create / reset */
    uint32_t flags;            /* VK_PROGRESS_* of create */
    uint64_t clamped_samples;  /* since create / reset (vk_stats.clamped_samples) */
} vk_progress_info;
int vk_progress_create(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t flags, vk_progress **out);
/* blocking; out: a host buffer as vk_render's.  stats_out: this window's samples, kernel time and clamped samples */
int vk_progress_step(vk_progress *pr, uint32_t n_samples, void *out, vk_stats *stats_out);
/* as vk_render_device: d_out on the scene's device (devices[0] of a multi-device scene), enqueued on hip_stream without a host wait */
int vk_progress_step_device(vk_progress *pr, uint32_t n_samples, void *d_out, void *hip_stream, vk_stats *stats_out);
/* back to sample 0 (waits for the last step); cam NULL = keep the camera */
int vk_progress_reset(vk_progress *pr, const vk_camera *cam);
/* The batch-means standard error of the current mean, per component (host buffer, width*height*3 floats, y up; this partition's pixels
 * only):   sqrt( (sum_j n_j m_j^2 - N m^2) / ((k - 1) N) )   with k the steps, n_j and m_j window j's length and own mean (from its exact
 * sum), N = samples_done and m the running mean.  Needs VK_PROGRESS_STDERR and k >= 2 (else VK_ERR_BAD_ARG); waits for the last step.
 * What it is NOT: it treats the windows as independent batches (they are: disjoint samples of independent RNG streams), but with k
 * windows it is itself an estimate from k - 1 degrees of freedom — noisy for small k (k = 4: about 40 % off in either direction) — and
 * a firefly (one bright sample) makes it heavy-tailed: its window's mean stands out, the estimate jumps, and a pixel whose fireflies
 * have not been drawn yet reports an error far too small.  Not on the hot path.                                                  */
int vk_progress_stderr(vk_progress *pr, float *out);
/* waits for the last step */
int vk_progress_get_info(vk_progress *pr, vk_progress_info *out);
void vk_progress_destroy(vk_progress *pr);   /* NULL: nothing */

/* ---- adaptive sampling (additive symbols of ABI 7) -----------------------------------------------------------------------------
 * Tiles whose error has converged stop; the others go on.  Adaptivity is per 8x8 tile of this call's partition, switched on for a
 * handle created with VK_PROGRESS_STDERR, before its first step since create / reset.  After every window each active tile is judged ON
 * THE DEVICE: a pixel has converged when for every component c
 *     v_c <= (abs_tol + rel_tol * |mean_c|)^2,   mean_c = run_c / 2^26 / N,   v_c = (m2_c - N * mean_c * mean_c) / ((k - 1) * N)
 * — the variance vk_progress_stderr squares, evaluated in double with its operation order (no contraction), N = samples_done and k =
 * steps.  A tile converges when all its in-image pixels have, with N >= min_samples and k >= min_steps.  A converged tile is FROZEN
 * until reset: it renders no more samples and its pixels keep being written with their frozen mean; every preview is complete.  The
 * active tiles share one count, samples_done; the budget check stays samples_done + n <= budget.
 *
 * Bit-identity.  After any sequence of steps, a pixel of tile t is, bit for bit, vk_render's pixel at samples_per_pixel = N_t (same
 * seed), N_t the tile's count (vk_progress_tile_samples) — f32 and RGB8, exact when clamped_samples == 0 (the clamp is the budget's).
 * vk_progress_stderr uses each tile's own N_t and k_t.  When no tile is active a step renders nothing, leaves the image as it was and
 * returns VK_OK; samples_done still advances (it counts the windows' samples), no tile's count changes.
 * vk_stats.samples of a step: exact from vk_progress_step; from vk_progress_step_device it is the count the host last learned (the
 * previous window's, if it has finished, else the partition's) — vk_adaptive_info.samples_rendered is always exact.
 * Tightening the tolerance later and resuming frozen tiles are not offered.  vk_progress_reset makes every tile active again and keeps
 * the parameters.                                                                                                                   */
typedef struct vk_adaptive_params {
    float abs_tol, rel_tol;      /* per component: stderr_c <= abs_tol + rel_tol * |mean_c|  (finite, >= 0) */
    uint32_t min_samples;        /* no tile stops with fewer samples ... */
    uint32_t min_steps;          /* ... or fewer windows (>= 2: the estimate needs two) */
} vk_adaptive_params;
/* VK_ERR_BAD_ARG, the handle unchanged: a null handle or ap, a handle without VK_PROGRESS_STDERR, min_steps < 2, a negative or non-finite
 * tolerance, a call after a step (since create / reset).  Called again before the first step: the new parameters. */
int vk_progress_set_adaptive(vk_progress *pr, const vk_adaptive_params *ap);
typedef struct vk_adaptive_info {
    uint32_t tiles_total;        /* tiles of this partition */
    uint32_t tiles_active;       /* of them not frozen (all of them without vk_progress_set_adaptive) */
    uint64_t samples_rendered;   /* pixel-samples in the running sums, summed over the partition's in-image pixels */
} vk_adaptive_info;
/* per tile of the image (tiles_x * tiles_y, row-major, tile row 0 = bottom like the f32 image): samples in its running sums, 0 outside
 * the partition; out and info may each be NULL.  Any handle (without adaptivity every tile has samples_done).  Waits for the last step. */
int vk_progress_tile_samples(vk_progress *pr, uint32_t *out, vk_adaptive_info *info);

/* ---- first-hit buffers, "AOVs" (additive symbols of ABI 7) ----------------------------------------------------------------------
 * replaces: nothing (the reference writes radiance only).  The first hit's albedo, normal, depth and coverage of exactly the primary rays
 * that vk_render's radiance samples use — what a denoiser or a compositor takes next to the noisy colour.  Per pixel of this call's tile
 * partition (pixels outside it are left untouched), in vk_render's f32 layout (y = 0 the bottom row): albedo and normal 3 floats per
 * pixel, depth and coverage 1.  Any of the four buffers may be NULL (not wanted), not all four.
 *   Samples.  first_sample .. first_sample + spp - 1, spp = params->samples_per_pixel.  Sample s is the primary ray of radiance sample s
 *     (stream (seed, pixel, s), camera draws first); a ConstantMedium draws its distance from that same stream after them, so sample s
 *     sees the first hit radiance sample s sees.
 *   First hit.  BVHNode::hit (accel.rs:58-83) with tmin 0.001, tmax inf on the tree AS HANDED OVER, also where vk_render walks a rebuilt
 *     one (exact re-treeing: the tree its second launch walks; none of the rebuilt forms is used).  A VK_SCENE_FAST_ACCEL scene keeps no
 *     copy of the tree as handed over on the device: there the rebuilt tree (the one vk_render walks, ties as the reference breaks them)
 *     is walked.
 *   Albedo of a hit: Lambertian / Metal / Isotropic the texture value at (u, v, p); Dielectric (1,1,1); DiffuseLight emitted(rec) (front
 *     faces only, material.rs:218-225) clamped to [0, 1]; SpecDiffuse pct * A(specular) + (1 - pct) * A(diffuse) in f32, recursively,
 *     0 below 8 SpecDiffuse levels.  A miss: the background the radiance sees (sky or solid), clamped to [0, 1].
 *   Normal of a hit: HitRec.normal in world space, face-oriented (set_face_normal); (0,0,0) for a medium hit and for a miss.
 *   Depth of a hit: t * |d| in f32, the distance from the sample's ray origin.
 *   Dropped samples: a sample with a non-finite albedo, normal or depth component adds to no sum and not to `hits`, but counts in n = spp.
 *   Aggregation, exact and in a fixed order: f32 sums in increasing sample order, then albedo = sum / (float)n, normal = sum / (float)n
 *     (misses included, not renormalised), depth = sum / (float)hits or +INFINITY without a hit, coverage = (float)hits / (float)n.  One
 *     value per (scene, camera, seed, window), whatever the launch shape.
 *   Arguments: vk_render's checks (null pointers, size, spp in 1..2^26, time0 < time1, ranges, tile_rank < tile_world), and also
 *     VK_ERR_BAD_ARG with nothing enqueued for output_format != VK_OUTPUT_F32, four NULL buffers, first_sample + spp > 2^32 - 1.
 *     max_depth and integrator are ignored.
 *   Scene state: "at most one render in flight per vk_scene" covers these calls too.  They touch nothing that describes vk_render's last
 *     frame (vk_scene_last_kernel_ms, the clamped and requeued counts, vk_debug_last_launches, the rebuilt tree's suspension) and no
 *     vk_progress handle.  stats_out: the AOV samples traced (partition pixels x spp), kernel_ms (vk_render_aov only), kernel_launches;
 *     clamped_samples = 0, scene_in_lds = 0 (the walk reads global memory).
 *   Multi-device scenes: the whole call runs on devices[0].                                                                      */
int vk_render_aov(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                  float *albedo, float *normal, float *depth, float *coverage, vk_stats *stats_out);
/* device buffers on the scene's device (devices[0] of a multi-device scene), enqueued on hip_stream, no host wait */
int vk_render_aov_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                         void *d_albedo, void *d_normal, void *d_depth, void *d_coverage, void *hip_stream, vk_stats *stats_out);

/* ---- specular guides: the buffers above, followed through mirrors and glass (additive symbols of ABI 7) ---------------------------
 * replaces: nothing.  vk_render_aov stops at the first hit: a glass sphere is albedo (1,1,1) with a smooth normal, a polished metal one
 * tint, and what is seen in or through them reaches a denoiser or a reprojection unguided.  vk_render_guides follows perfect-specular
 * ("delta") interactions to the first surface that is not one and reports THAT surface.  vk_render_aov is unchanged.
 * Layouts, the sample window, the tile partition, the argument checks, the scene-state rules, the multi-device rule and stats_out are
 * vk_render_aov's; `bounces` is a fifth optional buffer, 1 float per pixel; any of the five may be NULL, not all five.  Also
 * VK_ERR_BAD_ARG with nothing enqueued: a null gp, max_bounces > 8, fuzz_max not finite or < 0, flags != 0.
 * Per sample s of pixel p, everything f32 and unfused in the reference's order:
 *   Segment 0 is vk_render_aov's: the primary ray of radiance sample s and its first hit, on the same tree view (a medium's draw
 *     continues the sample's stream).  thr = (1,1,1), len = 0, b = 0.
 *   Delta hit: the closest hit is not a medium's, and its material is Dielectric, or Metal with fuzz <= fuzz_max.  (A SpecDiffuse is
 *     not a delta material, whatever its children.)
 *   Continuation, while the hit is a delta hit and b < max_bounces: len += t * |d| (|d| = sqrtf(d.d), as the depth rule has it); the next
 *     ray starts at rec.p with the sample's time; Metal: direction reflect(unit(d), n) (material.rs:118-132 without the fuzz term),
 *     thr = thr * texture value at (u, v, p); Dielectric: exactly the operations of material.rs:150-175 with the Schlick draw skipped
 *     — eta = front ? 1 / ir : ir, cos = fminf(dot(-unit(d), n), 1), sin = sqrtf(1 - cos * cos), reflect when eta * sin > 1, refract
 *     (util.rs:18-23) otherwise — thr unchanged; b += 1; BVHNode::hit with tmin 0.001, tmax inf on the same tree view.  A
 *     ConstantMedium met on continuation segment b (1..8) draws from a fresh stream rng_for_sample(cseed, 0, 0), cseed = seed +
 *     0x9E3779B97F4A7C15 * ((((u64)pixel << 32) | sample) * 16 + b) in wrapping u64.
 *   Terminal surface, the last surface hit: a continuation segment that misses leaves the delta hit it started from as the terminal
 *     surface — normal that hit's, depth = len (which holds the segment that reached it), albedo = thr * clamp01(background(direction of
 *     the missing segment)), the sky unitised as for a first-hit miss.  Otherwise albedo = thr * (the first-hit albedo rule at the
 *     terminal hit), normal by the first-hit rule ((0,0,0) for a medium), depth = len + t * |d|.  A primary miss is vk_render_aov's.
 *     `hit` is the primary ray's: coverage equals vk_render_aov's.
 *   Dropped samples and aggregation are vk_render_aov's; bounces = (sum of b over the kept samples, as an integer) / (float)n.
 *   max_bounces = 0 returns vk_render_aov's four buffers bit for bit.
 * What this is not.  The depth is the unfolded path length, a "virtual" depth: reprojecting with it is right for a planar mirror and
 * only approximate for a curved one (the virtual image of a curved mirror does not lie at that distance).  Glass shows its refraction
 * only, never its Fresnel reflection: the Schlick-weighted choice is not drawn, so a pane's faint mirror image has no guide.  One
 * path per sample: no separate reflection and refraction layers, no motion vectors.                                              */
typedef struct vk_guide_params {
    uint32_t max_bounces;        /* continuations per sample, 0..8 */
    float fuzz_max;              /* a Metal of fuzz <= fuzz_max is a mirror */
    uint32_t flags;              /* 0 */
} vk_guide_params;
/* max_bounces 4, fuzz_max 0, flags 0; touches no device */
int vk_guide_default_params(vk_guide_params *out);
int vk_render_guides(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                     const vk_guide_params *gp, float *albedo, float *normal, float *depth, float *coverage, float *bounces,
                     vk_stats *stats_out);
/* device buffers on the scene's device (devices[0] of a multi-device scene), enqueued on hip_stream, no host wait */
int vk_render_guides_device(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                            const vk_guide_params *gp, void *d_albedo, void *d_normal, void *d_depth, void *d_coverage, void *d_bounces,
                            void *hip_stream, vk_stats *stats_out);

/* ---- ray queries: closest hits for caller-supplied rays (additive symbols of ABI 7) -------------------------------------------------
 * replaces: world.hit(&ray, 0.001, tmax) of main.rs:130, for rays the CALLER supplies (autofocus, picking, collision of an orbiting
 * camera, visibility probes, a wavefront integrator of the caller's own).  Ray i of the batch gives the result of
 * BVHNode::hit(&Ray{origin, direction, time}, 0.001, tmax) (accel.rs:58-83), everything f32 and unfused in the reference's order.
 *   Tree view.  The one vk_render_aov walks: the tree AS HANDED OVER, also where vk_render walks a grid, a near or a unit form; under
 *     VK_SCENE_FAST_ACCEL the rebuilt tree (ties as the reference breaks them).
 *   tmin is 0.001 (VK_RAY_TMIN) for every ray, as at every call site of the reference; there is no per-ray tmin.
 *   tmax.  The closest-so-far distance starts at the ray's tmax instead of infinity.  With nothing accepted yet a Rect at exactly tmax is
 *     accepted (hittable.rs:232 rejects `t > tmax` only) and a Sphere, a MovingSphere or a Boxy / list is not (hittable.rs:75, :386).  A
 *     ray whose tmax is a NaN or <= VK_RAY_TMIN misses without a walk.  +INFINITY is main.rs:130's call.
 *   Media.  A ConstantMedium met by ray i draws from the stream rng_for_sample(seed + 0x9E3779B97F4A7C15 * (first_index + i), 0, 0), in
 *     wrapping u64: one fresh stream per ray.  A batch cut into pieces whose first_index continue each other gives the same bytes.
 *   The record of a hit is the reference's HitRec in world space: p, normal (face-oriented, set_face_normal), t, u, v (Sphere and
 *     MovingSphere: get_sphere_uv, always; Rect and Boxy faces: the rect's; a medium: its boundary's entry hit's), front; `material` the
 *     description's material index; `medium` = 1 when ConstantMedium::hit filled the record (normal (1,0,0), front 1).  `object` names the
 *     record of the description whose own hit() produced the winner, as a vk_ref with the flip bit clear: VK_KIND_SPHERE,
 *     VK_KIND_MOVING_SPHERE or VK_KIND_RECT and its index — for a face of a Boxy the vk_rect of that side of its list — or, for a medium
 *     hit, VK_KIND_MEDIUM and the vk_medium's index.
 *   A miss: hit = 0, t = +INFINITY, every other field 0.
 *   Non-finite rays are the reference's: a NaN or infinite component passes every AxisBB::hit (f32::min / max drop the NaN quotients)
 *     and fails every Sphere::hit, so in a world of spheres the ray misses (without a walk).  Rect::hit rejects with `<` and `>` only, which
 *     a NaN passes: such a ray can "hit" a Rect with a NaN t, here as there.  direction is not normalised and may be zero (a miss on
 *     spheres).
 *   Arguments: VK_ERR_BAD_ARG with nothing enqueued and the outputs untouched for a null scene or params, null rays or hits with n_rays
 *     > 0, flags != 0, n_rays > 2^32.  n_rays == 0: VK_OK, nothing done (stats_out zeroed).
 *   Scene state: vk_render_aov's rules.  The call is the scene's one render in flight; it touches nothing that describes vk_render's last
 *     frame and no vk_progress or vk_temporal handle.  A multi-device scene runs the call on devices[0].  stats_out: samples = n_rays,
 *     kernel_ms (vk_trace_rays only: summed over its chunks), kernel_launches, scene_in_lds = 0.
 *   vk_trace_rays stages rays and hits through scratch of the scene handle (allocated on first use, regrown, at most 2^20 rays at a time:
 *     longer batches run in chunks, which first_index makes invisible).  The first ray query of a scene also uploads the tables that map
 *     device primitives back to the description (4 bytes per sphere, moving sphere, rect and medium, 24 per Boxy).                    */
#define VK_RAY_TMIN 0.001f            /* the reference's tmin at every call site (main.rs:130) */
typedef struct vk_ray {               /* 32 bytes */
    float origin[3]; float tmax;
    float direction[3]; float time;   /* not normalised, as Ray (main.rs:32-36) */
} vk_ray;
typedef struct vk_hit {               /* 64 bytes */
    float p[3]; float t;
    float normal[3]; float u;
    float v; uint32_t hit; uint32_t front; uint32_t material;
    vk_ref object; uint32_t medium; uint32_t _pad[2];
} vk_hit;
typedef struct vk_trace_params {
    uint64_t seed;               /* of the media's streams */
    uint64_t first_index;        /* index of rays[0] in the caller's batch */
    uint32_t flags;              /* 0 */
    uint32_t _pad;
} vk_trace_params;
int vk_trace_rays(vk_scene *scene, const vk_trace_params *params, const vk_ray *rays, uint64_t n_rays, vk_hit *hits,
                  vk_stats *stats_out);
/* device buffers on the scene's device (devices[0] of a multi-device scene), 16-byte aligned, enqueued on hip_stream, no host wait */
int vk_trace_rays_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_hits,
                         void *hip_stream, vk_stats *stats_out);

/* ---- occlusion queries: any-hit for caller-supplied rays (additive symbols of ABI 7) --------------------------------------------------
 * replaces: world.hit(&ray, 0.001, tmax).is_some(), for the shadow and visibility rays of the ray queries' users.
 *   occluded[i] = 1 if BVHNode::hit(&Ray{origin, direction, time}, 0.001, tmax) returns Some, else 0.
 *   THE CONTRACT: occluded[i] equals hits[i].hit of vk_trace_rays called with the same scene, params and rays, bit for bit, for every
 *     ray, media included.  (BVHNode::hit only ever replaces an accepted hit with a closer one, so Some is decided at the first
 *     acceptance; the walk stops there, after the same steps and — in a ConstantMedium — the same draws of the same stream.)
 *   Everything else is vk_trace_rays' rule: tmin is VK_RAY_TMIN; a tmax that is a NaN or <= VK_RAY_TMIN gives 0 without a walk; with
 *     nothing accepted a Rect at exactly tmax counts and a Sphere, a MovingSphere or a Boxy does not; non-finite rays are the
 *     reference's (a NaN ray that "hits" a Rect with a NaN t is occluded = 1); the tree view; the stream of ray i,
 *     rng_for_sample(seed + 0x9E3779B97F4A7C15 * (first_index + i), 0, 0); the scene-state rules (the scene's one render in flight,
 *     nothing of vk_render's last frame, no vk_progress or vk_temporal handle touched); devices[0] of a multi-device scene.
 *   Segment visibility between two points a and b is the ray origin = a, direction = b - a, tmax = 1: it needs no further call.
 *   Arguments: VK_ERR_BAD_ARG with nothing enqueued and the outputs untouched for a null scene or params, null rays or occluded with
 *     n_rays > 0, flags != 0, n_rays > 2^32.  n_rays == 0: VK_OK, nothing done (stats_out zeroed).  Bytes beyond occluded[n_rays - 1]
 *     are never written.
 *   stats_out: samples = n_rays, kernel_ms (vk_trace_occluded only: summed over its chunks), kernel_launches.
 *   vk_trace_occluded stages rays and bytes through the ray queries' scratch of the scene handle, at most 2^20 rays at a time (longer
 *     batches run in chunks, which first_index makes invisible).  No tables are uploaded: the call names no object.               */
int vk_trace_occluded(vk_scene *scene, const vk_trace_params *params, const vk_ray *rays, uint64_t n_rays, uint8_t *occluded,
                      vk_stats *stats_out);
/* device buffers on the scene's device (devices[0] of a multi-device scene): d_rays 16-byte aligned, d_occluded (n_rays bytes) of any
 * alignment; enqueued on hip_stream, no host wait */
int vk_trace_occluded_device(vk_scene *scene, const vk_trace_params *params, const void *d_rays, uint64_t n_rays, void *d_occluded,
                             void *hip_stream, vk_stats *stats_out);

/* ---- radiance queries: path-traced colour for caller-supplied rays (additive symbols of ABI 7) ---------------------------------------
 * replaces: ray_color(&ray, &background, &world, &lights, 1) of main.rs:123-153 (ray_color_scatter for VK_INTEGRATOR_SCATTER), for rays
 * the CALLER supplies: a panorama or environment-map bake, a fisheye or orthographic camera, a lightmap texel, an irradiance probe, a
 * camera model of the caller's own.  rgb_out[i] is the mean of samples_per_ray samples of ray i.
 *   Sample s of ray i, s in [first_sample, first_sample + samples_per_ray), is ray_color(&Ray{origin, direction, time}, depth 1) with the
 *     scene's lights, the given background and max_depth, everything f32 and unfused in the reference's order: exactly what vk_render
 *     computes for a sample once it has its primary ray.  Its stream is rng_for_sample(seed + 0x9E3779B97F4A7C15 * (first_index + i), 0,
 *     s), in wrapping u64, taken from its beginning.  The ray is the same for every sample: a caller who wants jitter (antialiasing, a
 *     lens, motion blur) supplies one ray per jittered sample.
 *   tmax replaces infinity in the FIRST world.hit only, by vk_trace_rays' rules: a tmax that is a NaN or <= VK_RAY_TMIN misses without
 *     a walk, and the path sees the background; with nothing accepted a Rect at exactly tmax is accepted and a Sphere, a MovingSphere
 *     or a Boxy is not.  Later segments use infinity.  Hence: the first segment of sample 0 is, media draws included, exactly what
 *     vk_trace_rays reports for the same seed, first_index and ray.
 *   Tree view.  The one vk_trace_rays walks: the tree as handed over, or under VK_SCENE_FAST_ACCEL the rebuilt one.
 *   Aggregation is vk_render's: a sample with a non-finite component adds nothing but counts in n (main.rs:192-194); sums are 64-bit
 *     fixed point with 2^-26 resolution; a component beyond +-min(1e10, 1.3e11 / samples_per_ray) is clamped to that and the sample
 *     counted in stats_out->clamped_samples; rgb_out[i] = sum / samples_per_ray.  The result is ONE value per (scene, params, ray,
 *     index): it does not depend on the launch shape, on the order of the rays or on how a batch is cut into pieces whose first_index
 *     continue each other.
 *   max_depth = 0: every sample is (0,0,0), as for vk_render.
 *   Arguments: VK_ERR_BAD_ARG with nothing enqueued and the outputs untouched for a null scene or params, null rays or rgb_out with
 *     n_rays > 0, flags != 0, samples_per_ray outside 1..2^26, first_sample + samples_per_ray > 2^32 - 1, an unknown integrator or
 *     background, n_rays > 2^32.  VK_ERR_UNSUPPORTED where vk_render answers it (the PDF integrator without lights, the scatter
 *     integrator with a SpecDiffuse).  n_rays == 0: VK_OK, nothing done (stats_out zeroed).
 *   Scene state: vk_trace_rays' rules.  The call is the scene's one render in flight; it touches nothing that describes vk_render's last
 *     frame and no vk_progress or vk_temporal handle.  A multi-device scene runs the call on devices[0].  Rays and colours are staged
 *     through the ray queries' scratch of the scene handle, at most 2^20 rays at a time (longer batches run in chunks, which first_index
 *     makes invisible).  stats_out: samples = n_rays * samples_per_ray, kernel_ms (summed over the chunks), kernel_launches (one per
 *     chunk), clamped_samples.
 *   There is no device-pointer variant yet.                                                                                         */
typedef struct vk_radiance_params {
    uint64_t seed;
    uint64_t first_index;        /* index of rays[0] in the caller's batch */
    uint32_t samples_per_ray;    /* 1..2^26 */
    uint32_t first_sample;       /* first_sample + samples_per_ray <= 2^32 - 1 */
    uint32_t max_depth;          /* as vk_render_params.max_depth (0: every sample (0,0,0)) */
    uint32_t integrator;         /* VK_INTEGRATOR_* */
    uint32_t background;         /* VK_BACKGROUND_* */
    float background_color[3];
    uint32_t flags;              /* 0 */
    uint32_t _pad;
} vk_radiance_params;
int vk_trace_radiance(vk_scene *scene, const vk_radiance_params *params, const vk_ray *rays, uint64_t n_rays,
                      float *rgb_out /* n_rays * 3 */, vk_stats *stats_out);

/* ---- irradiance queries: cosine-weighted radiance at caller-supplied points (additive symbols of ABI 7) ------------------------------
 * replaces: CosinePDF::new(n).generate() (util.rs:126-130, 144-146) followed by ray_color, for surface points the CALLER supplies: a
 * lightmap texel, an irradiance probe, an ambient term.  rgb_out[i] is the mean radiance arriving at point i over cosine-weighted
 * directions of the hemisphere around its normal.  The directions are drawn on the device from each sample's own stream: the caller
 * uploads 32 bytes per point, not per sample, and keeps sample windows and the one-value guarantee of vk_trace_radiance.
 *   A point is a vk_ray read as: origin = the position p; direction = the surface normal n, of any non-zero length (the hemisphere is
 *     the one around n as given: the call is one-sided); time = the time of every ray from the point; tmax cuts the first segment only,
 *     by vk_trace_radiance's rule (a finite tmax gives a range-limited gather: what lies beyond it is the background).
 *   Sample s of point i, s in [first_sample, first_sample + samples_per_ray), everything f32 and unfused in the reference's order:
 *     g = rng_for_sample(seed + 0x9E3779B97F4A7C15 * (first_index + i), 0, s), in wrapping u64, taken from its beginning;
 *     local = random_cosine_direction(g) (util.rs:52-63: two gen_f32 draws, so the stream's counter stands at 2);
 *     d = ONB::new_from_w(n).local(local) (util.rs:95-110), not normalised afterwards;
 *     the sample is ray_color(&Ray{p, d, time}, depth 1) CONTINUING the stream g (ray_color_scatter for VK_INTEGRATOR_SCATTER), tmax
 *     the closest-so-far distance of its first world.hit.  Everything behind that is vk_trace_radiance's rule word for word: the tree
 *     view, VK_RAY_TMIN, media draws from the sample's stream.  max_depth = 0: every sample is (0,0,0) and nothing is drawn.
 *   Aggregation is vk_trace_radiance's: a sample with a non-finite component adds nothing but counts in n; sums are 64-bit fixed point
 *     with 2^-26 resolution; a component beyond +-min(1e10, 1.3e11 / samples_per_ray) is clamped to that and the sample counted in
 *     stats_out->clamped_samples; rgb_out[i] = sum / samples_per_ray.  The result is ONE value per (scene, params, point, index): it
 *     does not depend on the launch shape, on the order of the points or on how a batch is cut into pieces whose first_index continue
 *     each other.
 *   What the value is.  The plain mean of the samples' radiance.  The directions' density cos / pi cancels the cosine of the irradiance
 *     integral, so the irradiance is E = pi * rgb_out[i], and a Lambertian texel of albedo a radiates a * rgb_out[i].  The library does
 *     not multiply by pi: the result stays the exact fixed-point mean.
 *   Degenerate normals get no special case.  ONB::new_from_w of a zero or non-finite normal has NaN axes; the ray is then non-finite and
 *     follows vk_trace_rays' rule for non-finite rays.  In a world of spheres only such a point sees the background along a NaN
 *     direction: VK_BACKGROUND_SOLID gives background_color exactly, VK_BACKGROUND_SKY gives NaN samples, which are dropped, so the
 *     result is (0,0,0).
 *   Arguments, VK_ERR_UNSUPPORTED, n_points == 0, scene state, multi-device scenes, staging (at most 2^20 points at a time through the
 *     ray queries' scratch) and stats_out (samples = n_points * samples_per_ray) are vk_trace_radiance's, with the same messages.
 *   There is no device-pointer variant yet.                                                                                         */
int vk_trace_irradiance(vk_scene *scene, const vk_radiance_params *params, const vk_ray *points, uint64_t n_points,
                        float *rgb_out /* n_points * 3 */, vk_stats *stats_out);

/* ---- probe queries: spherical-harmonic radiance at caller-supplied points (additive symbols of ABI 7) -------------------------------
 * replaces: random_in_unit_sphere().unit_vector() (util.rs:31-39) followed by ray_color, for points the CALLER supplies that have no
 * normal: a light probe of an irradiance volume, the lighting of a moving object.  sh_out holds, per probe, the mean over uniformly
 * distributed directions of the incoming radiance times each of the nine real spherical-harmonic basis functions of bands 0..2, per
 * colour channel: 27 floats, from which vk_probe_eval answers for ANY normal afterwards.  The directions are drawn on the device from
 * each sample's own stream: the caller uploads 32 bytes per probe and downloads 108.
 *   A probe is a vk_ray read as: origin = the position p; direction is NOT READ (any bytes, NaN included, give the same result);
 *     time = the time of every ray from the probe; tmax cuts the first segment only, by vk_trace_radiance's rule: a tmax that is a NaN
 *     or <= VK_RAY_TMIN misses without a walk, and the sample is the background along its direction.
 *   Sample s of probe i, s in [first_sample, first_sample + samples_per_ray), everything f32 and unfused in the reference's order:
 *     g = rng_for_sample(seed + 0x9E3779B97F4A7C15 * (first_index + i), 0, s), in wrapping u64, taken from its beginning;
 *     b = random_in_unit_sphere(g) (util.rs:31-39: x, y, z = three gen_range(-1, 1) draws in this order, again while
 *       (x*x + y*y) + z*z >= 1, so the stream's counter stands at 3 * tries);
 *     u = b.unit_vector() = (b.x / l, b.y / l, b.z / l) with l = sqrtf((b.x*b.x + b.y*b.y) + b.z*b.z);
 *     the sample is L = ray_color(&Ray{p, u, time}, depth 1) CONTINUING the stream g (ray_color_scatter for VK_INTEGRATOR_SCATTER), tmax
 *     the closest-so-far distance of its first world.hit.  Everything behind that is vk_trace_radiance's rule word for word: the tree
 *     view, VK_RAY_TMIN, media draws from the sample's stream.  max_depth = 0: every sample is (0,0,0) and nothing is drawn.
 *   Basis.  With (x, y, z) = u, in f32 in exactly this form:
 *     Y0 = 0.282095f              Y1 = 0.488603f*y            Y2 = 0.488603f*z
 *     Y3 = 0.488603f*x            Y4 = 1.092548f*(x*y)        Y5 = 1.092548f*(y*z)
 *     Y6 = 0.315392f*(3.0f*(z*z) - 1.0f)                      Y7 = 1.092548f*(x*z)        Y8 = 0.546274f*(x*x - y*y)
 *   Aggregation.  The contribution of a sample to coefficient k, channel c is the f32 product Y_k * L_c.  A sample with a non-finite
 *     component of L or of u adds to none of the 27 sums but counts in n = samples_per_ray (a zero b gets no special case: its NaN
 *     direction drops the sample).  Sums are 64-bit fixed point with 2^-26 resolution: each product is clamped to
 *     +-min(1e10, 1.3e11 / samples_per_ray), multiplied by 2^26 and truncated toward zero; a sample with at least one clamped product
 *     counts once in stats_out->clamped_samples.  sh_out[(i * 9 + k) * 3 + c] = (float)sum * 2^-26 / (float)samples_per_ray, each step
 *     in f32.  The result is ONE value per (scene, params, probe, index): it does not depend on the launch shape, on the order of the
 *     probes, on how a batch is cut into pieces whose first_index continue each other, or on how the samples are split over launches
 *     (the fixed-point sums of two sample windows add).
 *   What the value is.  The plain mean of Y_k(u) * L(u) over the sphere's uniform density 1 / 4pi.  The spherical-harmonic coefficient
 *     of the radiance is therefore 4pi * sh_out.  The library does not multiply by 4pi: the result stays the exact fixed-point mean, and
 *     vk_probe_eval's weights contain the factor.
 *   Arguments, VK_ERR_UNSUPPORTED, n_probes == 0, scene state, multi-device scenes, staging (at most 2^20 probes at a time through the
 *     ray queries' scratch) and stats_out (samples = n_probes * samples_per_ray) are vk_trace_radiance's, with the same messages.
 *   There is no device-pointer variant yet.                                                                                         */
#define VK_PROBE_COEFFS 9u
int vk_trace_probes(vk_scene *scene, const vk_radiance_params *params, const vk_ray *probes, uint64_t n_probes,
                    float *sh_out /* n_probes * 9 * 3 */, vk_stats *stats_out);
/* Evaluates a probe for the direction n (of any non-zero length; normalised here).  Touches no device and no handle.
 *   rgb[c] = sum_k w_l(k) * sh27[k * 3 + c] * Y_k(unit(n)), l(k) the band of k (0; 1..3; 4..8), computed in double and rounded once.
 *   mode 0: the radiance arriving along n, band-limited: w = 4pi for every k.
 *   mode 1: irradiance / pi for a surface of normal n — the quantity vk_trace_irradiance's rgb_out estimates — by the cosine lobe's
 *     band weights: w_0 = 4pi, w_1 = 8pi/3, w_2 = pi.
 *   VK_ERR_BAD_ARG for a null pointer or another mode; rgb is then untouched.  A zero or non-finite n gives NaN.                    */
int vk_probe_eval(const float *sh27, const float n[3], uint32_t mode, float rgb[3]);

/* ---- shade queries: one bounce of ray_color on the caller's hits (additive symbols of ABI 7) ----------------------------------------
 * replaces: the body of ray_color (main.rs:123-153; ray_color_scatter for VK_INTEGRATOR_SCATTER) behind its world.hit, for a (ray, hit,
 * path state) the CALLER supplies: the other half of a wavefront integrator's loop around vk_trace_rays — per-bounce outputs, a
 * termination rule or next-event rays of the caller's own (through vk_trace_occluded), split paths — with the library's materials,
 * textures, light sampling and sky, and its samples.  Everything is f32 and unfused, in the reference's order.
 *   Item i is one call of that body with r.direction = rays[i].direction, r.time = rays[i].time (origin and tmax are not read), the
 *     throughput thr, the radiance so far acc and the depth of states[i] (`depth` as ray_color's argument: a fresh path has thr (1,1,1),
 *     acc (0,0,0), depth 1), and the stream rng_for_sample(seed, pixel, sample) standing at draw `counter` (fresh: 0); max_depth, the
 *     integrator and the background from params.
 *   Miss (hits[i].hit == 0): acc += thr * background(unit(direction)) — the direction is normalised only for the sky; status
 *     VK_SHADE_MISS; nothing is drawn.
 *   Hit (hits[i].hit == 1): the HitRec is p, normal, t, u, v, front != 0 and material of hits[i], the material
 *     materials[hits[i].material] of the description.  Then emitted, scatter / scatter_with_pdf (SpecDiffuse resolved by its draws), the
 *     mixture-PDF light sampling and the update of acc and thr exactly as vk_render makes them, the PDF integrator's time 0 for a Metal's
 *     ray included; then depth += 1, and a depth above max_depth ends the path with acc += thr * 0 (which keeps the reference's NaN).
 *     status VK_SHADE_SCATTERED with the next ray in `next` (origin = hits[i].p, tmax = +INFINITY), or VK_SHADE_ENDED (an emitter, an
 *     absorbing Metal, the depth) with `next` zeros.  `medium` needs no special case: an Isotropic material shades from the record.
 *     lobe: VK_MAT_* of the material finally sampled (the SpecDiffuse's child the draws chose); 0xFFFFFFFF for MISS and BAD_HIT.
 *   Bad hit (hits[i].hit > 1, or hit == 1 and material >= the description's n_materials): status VK_SHADE_BAD_HIT, the state copied
 *     through, `next` zeros, nothing drawn, and no memory read by that index.
 *   state: thr, depth, acc and counter after the bounce; seed, pixel and sample copied.  _pad is written 0.
 *   THE CONTRACT.  In a scene without a ConstantMedium (vk_trace_rays then draws nothing): start ray i of a batch with the state {thr 1,
 *     depth 1, acc 0, counter 0, seed + 0x9E3779B97F4A7C15 * (first_index + i) in wrapping u64, pixel 0, sample s}, then repeat
 *     hits = vk_trace_rays(rays); out = vk_shade_hits(rays, hits, states); rays, states = out.next, out.state while status is
 *     VK_SHADE_SCATTERED.  state.acc then equals sample s of vk_trace_radiance for that ray, seed, first_index and parameters, before its
 *     finite filter, bit for bit (a NaN's payload aside), and state.counter its stream's final counter.  The first call uses the ray's
 *     own tmax; next.tmax is +INFINITY: vk_trace_radiance's "first segment only" rule.
 *     With media the loop is still a valid estimator but not that sample: vk_trace_rays draws a medium's distance from its own per-ray
 *     stream, not from the path's.  A path batch (vk_paths_*, below) traces on the path's stream and keeps the contract in every scene.
 *   max_depth = 0 gets no special case here: a hit at depth 1 ends with acc += thr * 0 and a miss adds the background.  The contract is
 *     for max_depth >= 1; vk_trace_radiance's (0,0,0) for max_depth = 0 starts no path at all, and neither should the caller.
 *   Arguments: VK_ERR_BAD_ARG with nothing enqueued and the outputs untouched for a null scene or params, a null rays, hits, states or
 *     out with n > 0, flags != 0, an unknown integrator or background, n > 2^32.  VK_ERR_UNSUPPORTED where vk_render answers it (the PDF
 *     integrator without lights, the scatter integrator with a SpecDiffuse), in the same words.  n == 0: VK_OK, nothing done (stats_out
 *     zeroed).
 *   Scene state: vk_trace_rays' rules.  The call is the scene's one render in flight; it touches nothing that describes vk_render's last
 *     frame and no vk_progress or vk_temporal handle.  A multi-device scene runs the call on devices[0].  Rays, hits, states and results
 *     are staged through the ray queries' scratch of the scene handle, at most 2^19 items at a time (longer batches run in chunks; an
 *     item's result depends on the item alone).  stats_out: samples = n, kernel_ms (summed over the chunks), kernel_launches.
 *   There is no device-pointer variant yet.                                                                                         */
typedef struct vk_path_state {        /* 48 bytes */
    float thr[3]; uint32_t depth;     /* throughput; depth as ray_color's (a fresh path: 1,1,1 and 1) */
    float acc[3]; uint32_t counter;   /* radiance so far; the stream's counter (fresh: 0) */
    uint64_t seed; uint32_t pixel, sample;   /* the stream rng_for_sample(seed, pixel, sample) */
} vk_path_state;
enum { VK_SHADE_MISS = 0, VK_SHADE_SCATTERED = 1, VK_SHADE_ENDED = 2, VK_SHADE_BAD_HIT = 3 };
struct vk_shaded {                    /* 96 bytes */
    vk_ray next;                      /* SCATTERED: origin = hit.p, tmax = +INFINITY, direction, time; else zeros */
    vk_path_state state;              /* the state after this bounce */
    uint32_t status;                  /* VK_SHADE_* */
    uint32_t lobe;                    /* VK_MAT_* of the material finally sampled (behind SpecDiffuse draws); 0xFFFFFFFF for MISS / BAD_HIT */
    uint32_t _pad[2];                 /* written 0 */
};
typedef struct vk_shaded vk_shaded;
typedef struct vk_shade_params {
    uint32_t max_depth;               /* as vk_render_params.max_depth */
    uint32_t integrator;              /* VK_INTEGRATOR_* */
    uint32_t background;              /* VK_BACKGROUND_* */
    float background_color[3];
    uint32_t flags;                   /* 0 */
    uint32_t _pad;
} vk_shade_params;
int vk_shade_hits(vk_scene *scene, const vk_shade_params *params, const vk_ray *rays, const vk_hit *hits,
                  const vk_path_state *states, uint64_t n, vk_shaded *out, vk_stats *stats_out);

/* ---- path batches: a device-resident wavefront loop (additive symbols of ABI 7) ------------------------------------------------------
 * replaces: the caller's loop around vk_trace_rays and vk_shade_hits, which stages 336 bytes per live path and bounce through the host
 * and compacts the survivors there.  A path batch is an opaque handle like vk_progress and vk_temporal: it owns rays, hits, states and
 * results on the scene's device (devices[0] of a multi-device scene), runs trace, shade and compact per bounce on the null stream, as
 * the host-pointer calls do, and moves one record of counts across the bus per bounce — more only when the caller asks (vk_paths_read,
 * vk_paths_cull, vk_paths_results).  No function takes a stream.  Destroy a batch before its scene.
 *   vk_paths_create: 1 <= capacity <= 2^24 paths.  Memory: 300 bytes a slot (ray 32, state 48, hit 64, vk_shaded 96, ids 2 x 4, result
 *     48 + 4) and the compaction's tables, 300 * capacity + 24 * ceil(capacity / 256) + 40 bytes of device memory in all; a failed
 *     allocation is VK_ERR_OOM and leaves *out untouched.
 *   vk_paths_begin: path i has the id i, the ray rays[i] and the state states[i], 0 <= i < n <= capacity; the live paths are kept in
 *     ascending id ("live order").  n == 0 is VK_OK with nothing live.  A handle may be begun again, which forgets the previous batch.
 *     params is checked as vk_shade_hits checks it, in the same words, VK_ERR_UNSUPPORTED where vk_render answers it included.
 *   vk_paths_step runs bounces until nothing is live or max_bounces of them are run (max_bounces == 0: VK_ERR_BAD_ARG).  One bounce,
 *     over the live paths:
 *     1. trace: vk_trace_rays' walk of the path's ray on the same tree view — tmin VK_RAY_TMIN, the ray's own tmax, vk_trace_rays' hit
 *        record and its rules for non-finite rays — except that a ConstantMedium met on the way draws from the PATH's stream,
 *        rng_for_sample(state.seed, state.pixel, state.sample) standing at state.counter, and state.counter advances by what was drawn:
 *        exactly what vk_trace_radiance does inside a sample.
 *     2. shade: vk_shade_hits' item, bit for bit, on that hit and the advanced state.
 *     3. retire and compact: a path whose status is not VK_SHADE_SCATTERED is retired — its state after the bounce and its status are
 *        stored under its id —, a scattered path continues with `next` and `state`.  The survivors keep their relative order (a stable
 *        compaction on the device), so live order stays ascending by id.
 *     info (may be NULL): traced = the rays walked, summed over the bounces run; live = the live paths after the call; missed, ended
 *     and bad = the paths this call retired with VK_SHADE_MISS, VK_SHADE_ENDED and VK_SHADE_BAD_HIT; bounces = run by this call;
 *     kernel_launches (five a bounce); kernel_ms between two events around each bounce's launches, summed; seconds of wall time.
 *   THE CONTRACT, in every scene, ConstantMedium included.  Begin with the states of vk_shade_hits' contract — thr 1, depth 1, acc 0,
 *     counter 0, seed + 0x9E3779B97F4A7C15 * (first_index + i) in wrapping u64, pixel 0, sample s — and step until nothing is live:
 *     the acc and counter of vk_paths_results' state i are sample s of vk_trace_radiance for that ray, seed, first_index and parameters,
 *     before that call's finite filter, bit for bit (a NaN's payload aside).  For max_depth >= 1; max_depth == 0 gets vk_shade_hits'
 *     treatment, no special case.
 *     In a scene without a ConstantMedium, moreover, vk_paths_read after every bounce returns byte for byte the live indices, out.next
 *     and out.state of the same bounce of the loop around vk_trace_rays and vk_shade_hits.
 *   vk_paths_read: the ids, rays and states of the live paths, in live order (vk_paths_info.live entries; any of the three may be NULL).
 *   vk_paths_cull: the caller's own termination rule (Russian roulette, a budget, a region of interest).  keep holds one byte per live
 *     path, in live order: a path with 0 is retired as VK_PATHS_CULLED with its state as it stands; a kept path's thr[c] becomes the f32
 *     product thr[c] * scale[j] where scale (one float per live path, or NULL) is given; the kept paths are compacted stably.  The call
 *     uploads 1 or 5 bytes per live path.  A NULL keep is VK_ERR_BAD_ARG when anything is live; with nothing live the call does nothing.
 *   vk_paths_results: per started id (vk_paths_info.started entries; either array may be NULL) a retired path's final state and its
 *     status — VK_SHADE_MISS, VK_SHADE_ENDED, VK_SHADE_BAD_HIT or VK_PATHS_CULLED —, a live path's current state and VK_PATHS_LIVE.
 *   vk_paths_get_info: capacity; started = the last begin's n; live; retired[status] since the last begin ([1] stays 0); bounces run
 *     since the last begin.  vk_paths_read, vk_paths_results and vk_paths_get_info wait for the handle's work.
 *   Arguments: VK_ERR_BAD_ARG with nothing enqueued and the outputs untouched for a null handle, scene, params, out or info pointer, a
 *     capacity out of range, null rays or states with n > 0, n > capacity, and vk_paths_step, vk_paths_cull or vk_paths_read before a
 *     vk_paths_begin.
 *   Scene state: vk_trace_rays' rules.  A call is the scene's one render in flight; it touches nothing that describes vk_render's last
 *     frame, not the launch log, no vk_progress or vk_temporal handle, and not the ray queries' scratch of the scene.  Two handles on
 *     one scene do not disturb each other.  vk_paths_destroy(NULL) does nothing.                                                      */
typedef struct vk_paths vk_paths;
enum { VK_PATHS_LIVE = 1 /* == VK_SHADE_SCATTERED */, VK_PATHS_CULLED = 4 };
typedef struct vk_paths_info {
    uint64_t capacity, started, live;
    uint64_t retired[5];              /* by status; [1] stays 0; [4]: culled, by vk_paths_cull / vk_regen_cull or the handle's roulette */
    uint32_t bounces, _pad;
} vk_paths_info;
typedef struct vk_paths_step_info {
    uint64_t traced;                  /* rays walked, summed over the bounces run */
    uint64_t live;                    /* after the call */
    uint64_t missed, ended, bad;
    uint32_t bounces;                 /* run by this call */
    uint32_t kernel_launches;
    double kernel_ms, seconds;
} vk_paths_step_info;
int vk_paths_create(vk_scene *scene, uint64_t capacity, vk_paths **out);
int vk_paths_begin(vk_paths *p, const vk_shade_params *params, const vk_ray *rays, const vk_path_state *states, uint64_t n);
int vk_paths_step(vk_paths *p, uint32_t max_bounces, vk_paths_step_info *info);
int vk_paths_read(vk_paths *p, uint32_t *ids, vk_ray *rays, vk_path_state *states);
int vk_paths_cull(vk_paths *p, const uint8_t *keep, const float *scale);
int vk_paths_results(vk_paths *p, vk_path_state *states, uint32_t *status);
int vk_paths_get_info(vk_paths *p, vk_paths_info *out);
void vk_paths_destroy(vk_paths *p);

/* ---- Russian roulette on the device for path batches and regenerating runs (additive symbols of ABI 7) -------------------------------
 * replaces: a throughput-based termination rule done through the host with vk_paths_read, vk_paths_cull / vk_regen_cull and a second
 * compaction per bounce (89 bytes per live path and bounce over the bus, and a regenerating run stepped one bounce a call).  The rule
 * is a property of the HANDLE: off after vk_paths_create, kept across vk_paths_begin, vk_film_emit and vk_regen_begin, and settable
 * between any two calls, mid-batch and mid-run too; it holds from the next bounce on.  It runs inside the compaction's count pass of
 * every bounce of vk_paths_step and vk_regen_step: no launch and no transfer is added (kernel_launches stays five a bounce, six with a
 * top-up), and with the rule off every kernel and launch is what it is without these symbols.
 *   The rule, everything f32, unfused, in this order.  A bounce's shaded record has state.depth after the bounce.  The rule applies to
 *     a record whose status is VK_SHADE_SCATTERED and whose state.depth >= first_depth:
 *     m = fmaxf(fmaxf(thr[0], thr[1]), thr[2])      (fmaxf drops a NaN)
 *     q = fminf(fmaxf(m, q_min), q_max)             (so q lies in [q_min, q_max], for NaN, infinite or negative throughputs too)
 *     u = the draw of a stream of the rule's own — the path's stream and state.counter are not touched: with key the key of
 *         rng_for_sample(state.seed ^ 0x52D1E7A9C3B5F04B, state.pixel, state.sample), u = gen_f32 of the value next_u32 returns from
 *         Rng{key, state.depth - 1}, that stream's draw number `depth`.
 *     u < q: the path goes on with thr[c] = thr[c] * (1.0f / q) — one IEEE division, then three products: vk_paths_cull's thr * scale
 *         with scale = 1.0f / q; q == 1 leaves thr bit for bit.
 *     otherwise the path is retired as VK_PATHS_CULLED with its state after the bounce as it stands, thr unscaled: vk_paths_step
 *         stores it under its id, vk_regen_step deposits it by vk_film_deposit's rule, vk_paths_info.retired[4] counts it.
 *   THE CONTRACT: a batch stepped with the rule set is, after every bounce and bit for bit, the batch stepped one bounce a call with
 *     the rule off that is given vk_paths_read, this rule on the host and vk_paths_cull (vk_regen_cull) after each bounce.
 *   vk_paths_cull and vk_regen_cull are unchanged and combine with the rule; vk_paths_step_info and vk_regen_info keep their layout.
 *   vk_roulette_set: rp == NULL turns the rule off.  VK_ERR_BAD_ARG, with the handle's setting left as it was, for a null
 *     handle, first_depth < 2, flags != 0, a non-finite q_min or q_max, and anything outside 2^-24 <= q_min <= q_max <= 1.
 *   vk_roulette_get: *enabled = 1 and *out = the rule where one is set, else 0 and zeros.  VK_ERR_BAD_ARG for a null pointer.  */
typedef struct vk_roulette_params {          /* 16 bytes */
    uint32_t first_depth;                    /* the first state.depth (after the bounce) the rule applies to; >= 2 */
    float q_min, q_max;                      /* 2^-24 <= q_min <= q_max <= 1 */
    uint32_t flags;                          /* 0 */
} vk_roulette_params;
int vk_roulette_set(vk_paths *p, const vk_roulette_params *rp);
int vk_roulette_get(vk_paths *p, vk_roulette_params *out, int *enabled);

/* ---- films: camera paths and frame sums for path batches, on the device (additive symbols of ABI 7) ----------------------------------
 * replaces: the caller's own camera (Camera::get_ray, the lens disk's rejection loop and the stream's counter behind them, restated bit
 * for bit), the 80 bytes per path vk_paths_begin uploads, the 52 bytes per path vk_paths_results downloads, and the finite filter, clamp
 * and fixed-point sums redone on the host.  A film is an opaque handle like a path batch: a frame's fixed-point accumulators on the
 * scene's device (devices[0] of a multi-device scene) together with its camera and render parameters.  It EMITS camera paths into a path
 * batch and DEPOSITS a finished batch into the frame, both on the device, on the null stream.  No function takes a stream.  Destroy a
 * film before its scene.
 *   vk_film_create: params is checked as vk_render checks it, in the same words, VK_ERR_UNSUPPORTED where vk_render answers it included.
 *     Refused besides, each VK_ERR_BAD_ARG: a tile partition other than the whole image (tile_world > 1), output_format other than
 *     VK_OUTPUT_F32, max_depth == 0 (vk_shade_hits' contract starts no path there), width * height > 2^26.  Memory: width * height * 24
 *     bytes of sums and one counter record of 32 bytes (and, from the first vk_film_resolve on, width * height * 12 bytes for the frame on
 *     its way to the host); a failed allocation is VK_ERR_OOM and leaves *out untouched.  The sums start at zero.
 *   vk_film_emit begins `batch` as vk_paths_begin does, forgetting its previous batch, with n = win.width * win.height * win.n_samples
 *     paths generated on the device: nothing crosses the bus.  Path id = ((y - y0) * win.width + (x - x0)) * n_samples + k is sample
 *     s = first_sample + k of pixel (x, y) of the film's frame: its ray is the render kernel's — the stream rng_for_sample(params.seed,
 *     y * width + x, s), the draws for u, v, the lens disk and the time, (float)(width - 1) and (float)(height - 1) of the FILM's frame —
 *     as origin, tmax = +INFINITY, the unnormalised direction and the time; its state is thr (1,1,1), depth 1, acc 0, seed = params.seed,
 *     pixel = y * width + x, sample = s, and counter = the stream's counter behind those draws.  The batch's shade parameters are the
 *     film's: max_depth, integrator, background.
 *     VK_ERR_BAD_ARG with nothing enqueued and the batch left as it was: a null pointer, a batch of another scene, an empty window, a
 *     window outside the frame, first_sample + n_samples > samples_per_pixel, n above the batch's capacity.
 *   vk_film_deposit adds the batch's retired paths to the film.  For every started id whose status is VK_SHADE_MISS, VK_SHADE_ENDED or
 *     VK_PATHS_CULLED the pixel is state.pixel of the RESULT, not the id — a batch begun by vk_paths_begin with the caller's own rays (a
 *     fisheye camera, a jitter of one's own) deposits too: the caller sets state.pixel.  pixel >= width * height: `skipped`, counted, no
 *     memory touched by that index.  An acc with a non-finite component: `dropped`, adds nothing (main.rs:192-194).  Otherwise the render
 *     kernel's conversion — 2^-26 fixed point, truncated; a sample with a component beyond 31.999 in magnitude is first clamped to
 *     +-min(1e10, 1.3e11 / samples_per_pixel) and, where that changed it, counted in `clamped` — and three additions to the pixel's 64-bit
 *     sums.  VK_SHADE_BAD_HIT results are `skipped`.
 *     VK_ERR_BAD_ARG: a batch with live paths (step or cull them first), a batch never begun, a batch of another scene, a batch already
 *     deposited since its last vk_paths_begin or vk_film_emit.  Emitting the same (pixel, sample) twice is the caller's error and is not
 *     detected.
 *   vk_film_resolve: rgb_out[(y * width + x) * 3 + c] = ((float)sum * 2^-26) / (float)n, vk_render's own arithmetic, into a host buffer in
 *     vk_render's f32 layout (y = 0 the bottom row).  n >= 1.  The call waits; it does not clear the sums.
 *   vk_film_reset zeroes the sums and the counters; cam may be NULL to keep the camera, otherwise it replaces it (checked as at create),
 *     as in vk_progress_reset.
 *   vk_film_get_info waits and returns the counters since the last reset: emitted = paths emitted, deposited + dropped + skipped = results
 *     read by the deposits, clamped (a part of deposited), deposits = calls.
 *   THE CONTRACT, on every scene whose vk_render is proven to equal the tree as handed over (everything but VK_SCENE_EMPIRICAL_TREES):
 *     1. after vk_film_emit and vk_paths_step until nothing is live, the acc and counter of vk_paths_results' state for an id are that
 *        sample of vk_render (vk_debug_render_samples' entry [pixel * samples_per_pixel + s]), bit for bit, a NaN's payload aside;
 *     2. once every (pixel, sample) with sample < samples_per_pixel has been emitted, finished and deposited exactly once — window shapes,
 *        batch sizes and order are free — vk_film_resolve(film, samples_per_pixel, out) is vk_render's f32 frame for the same camera
 *        and parameters BIT FOR BIT, and `clamped` is that call's clamped_samples;
 *     3. for n < samples_per_pixel deposited samples per pixel the image is vk_render's at n samples per pixel wherever no sample lies
 *        beyond either clamp.
 *   Scene state: the path batch's rules.  A call is the scene's one render in flight; it touches nothing that describes vk_render's last
 *     frame, not the launch log, no vk_progress or vk_temporal handle, and not the ray queries' scratch.  Two films and two batches on
 *     one scene do not disturb each other.  vk_film_destroy(NULL) does nothing.                                                       */
typedef struct vk_film vk_film;
typedef struct vk_film_window {          /* 24 bytes */
    uint32_t x0, y0, width, height;      /* a pixel rectangle inside the film's frame, y = 0 the bottom row */
    uint32_t first_sample, n_samples;    /* samples [first_sample, first_sample + n_samples) of each of its pixels */
} vk_film_window;
typedef struct vk_film_info {            /* 64 bytes */
    uint32_t width, height, samples_per_pixel, _pad;
    uint64_t emitted, deposited, dropped, clamped, skipped, deposits;
} vk_film_info;
int vk_film_create(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, vk_film **out);
int vk_film_emit(vk_film *film, vk_paths *batch, const vk_film_window *win);
int vk_film_deposit(vk_film *film, vk_paths *batch);
int vk_film_resolve(vk_film *film, uint32_t n, float *rgb_out);
int vk_film_reset(vk_film *film, const vk_camera *cam);
int vk_film_get_info(vk_film *film, vk_film_info *out);
void vk_film_destroy(vk_film *film);

/* ---- regeneration: a path batch refilled from a film's window as its paths retire (additive symbols of ABI 7) -------------------------
 * replaces: the caller's loop of windows, each emitted, stepped to its end and deposited (vk_film_emit, vk_paths_step, vk_film_deposit),
 * which walks the ever shorter tail of every window and needs a window to fit the batch.  A regenerating run sends a window of ANY number
 * of paths through a batch of ANY capacity: every bounce first tops the batch up with the window's next camera paths, and a path that
 * retires is deposited into the film there and then.  Only the last tail of a run is walked thin.  No function takes a stream; all work
 * is on the null stream, on the scene's device (devices[0] of a multi-device scene).
 *   The window's sequence.  Path number q = ((y - y0) * win.width + (x - x0)) * n_samples + k, 0 <= q < total = win.width * win.height *
 *     win.n_samples, is exactly path id q of vk_film_emit for the same window: the same ray and state, the same stream position behind
 *     the camera's draws.  Its id in the batch is q.  Ids are 32 bits: total >= 2^32 is VK_ERR_BAD_ARG (split the window by sample
 *     ranges).  total is not bounded by the batch's capacity.
 *   vk_regen_begin checks what vk_film_emit checks, in the same words, except the capacity rule, and puts `batch` into its REGENERATING
 *     state for this film and window: nothing live, next = 0, counters as after a begin, the film's shade parameters.  It enqueues
 *     nothing that emits.  It forgets a previous batch or run, as vk_paths_begin does.
 *   vk_regen_step runs bounces until the run is finished or max_bounces of them are run (max_bounces == 0: VK_ERR_BAD_ARG).  One bounce:
 *     1. top up: m = min(capacity - live, total - next) fresh paths next .. next + m go to slots live .. live + m, ids = their numbers;
 *        live += m, next += m;
 *     2. if nothing is live, the run is finished;
 *     3. trace and shade exactly as vk_paths_step does: the same kernels, the same tree view, the path's own stream through media;
 *     4. retire and compact: a path whose status is not VK_SHADE_SCATTERED is deposited into the film there and then, by
 *        vk_film_deposit's rule applied to its state after the bounce — VK_SHADE_MISS and VK_SHADE_ENDED at state.pixel, a non-finite acc
 *        `dropped`, both conversions and the clamp of the film's samples_per_pixel as there, VK_SHADE_BAD_HIT and a pixel outside the
 *        frame `skipped`.  Nothing is stored under its id.  The survivors are compacted stably to the front.
 *     The run is finished when live == 0 and remaining == 0.  A finished run leaves the batch begun, with nothing live and marked as
 *     deposited; a step on a finished run is VK_OK and does nothing.  info (may be NULL): see vk_regen_info; kernel_launches counts six
 *     a bounce, five where nothing was left to top up.
 *     The invariant: live order is ascending by id at every moment — the survivors keep their order, the top-up appends larger numbers.
 *   vk_regen_cull is vk_paths_cull's rule between two steps: keep and scale in live order, a kept path's thr scaled, a culled path
 *     deposited as VK_PATHS_CULLED with its state as it stands, as vk_film_deposit would, the kept paths compacted stably.  There is no
 *     top-up: the next step does it.
 *   Arguments: for each of the three calls VK_ERR_BAD_ARG with nothing enqueued and film and batch left as they were for a null pointer, a
 *     batch of another scene, for step and cull a batch that is not regenerating, and a film other than the one the run was begun with.
 *   Existing functions on a regenerating batch: vk_paths_read works (live ids, rays and states) and so does vk_paths_get_info (started =
 *     emitted so far, live, retired[], bounces); vk_paths_step, vk_paths_cull, vk_paths_results and vk_film_deposit are VK_ERR_BAD_ARG;
 *     vk_paths_begin and vk_film_emit end the run and forget what was live and what remained.  vk_film_reset or vk_film_destroy during
 *     a run is the caller's error and is not detected.
 *   vk_film_info: emitted grows by the top-ups; deposited, dropped, clamped and skipped by the retirements; deposits counts
 *     vk_film_deposit calls only.
 *   THE CONTRACT, on every scene where the film's contract holds:
 *     1. per path: the state a path retires with is the state the window route (vk_film_emit, vk_paths_step, vk_film_deposit) retires it
 *        with, bit for bit — a path's trajectory depends on its own state alone — so the sums are equal;
 *     2. per frame: once every (pixel, sample) with sample < samples_per_pixel went through exactly once — by regenerating runs, by the
 *        emit / deposit route, or both mixed across windows; any capacity >= 1, any slicing by max_bounces, any order —
 *        vk_film_resolve(film, samples_per_pixel, out) is vk_render's f32 frame BIT FOR BIT, and `clamped` is its clamped_samples;
 *     3. per bounce: after every bounce vk_paths_read returns ids, rays and states that are a function of the window, the capacity and
 *        the paths' lifetimes (the bounces until each retires) alone: the schedule is deterministic, nothing depends on how workgroups
 *        are scheduled.
 *   Scene state: the path batch's rules.  A call touches nothing that describes vk_render's last frame, not the launch log, no vk_progress
 *     or vk_temporal handle, and not the ray queries' scratch.                                                                          */
typedef struct vk_regen_info {          /* 80 bytes */
    uint64_t traced;                    /* rays walked, summed over the bounces run by this call */
    uint64_t live;                      /* after the call (before the next top-up) */
    uint64_t remaining;                 /* paths of the window not yet emitted */
    uint64_t emitted;                   /* by this call's top-ups */
    uint64_t missed, ended, bad;        /* retired by this call, by status */
    uint32_t bounces, kernel_launches;
    double kernel_ms, seconds;
} vk_regen_info;
int vk_regen_begin(vk_film *film, vk_paths *batch, const vk_film_window *win);
int vk_regen_step(vk_film *film, vk_paths *batch, uint32_t max_bounces, vk_regen_info *info);
int vk_regen_cull(vk_film *film, vk_paths *batch, const uint8_t *keep, const float *scale);

/* ---- a film's error moments and adaptive regeneration (vk_adapt_*, additive symbols of ABI 7) -----------------------------------------
 * replaces: nothing.  What vk_progress keeps next to its running sums — the batch-means moments behind vk_progress_stderr and the tile
 * map of vk_progress_set_adaptive — kept next to a film's sums, so that a frame made of path batches has an error estimate (the stderr3
 * image vk_denoise and vk_temporal_accumulate take) and stops sampling the 8x8 tiles that have converged.  The handle stays vk_film; a
 * film on which vk_adapt_enable was never called allocates and does what it did.  No call takes a stream: all work is on the null stream
 * of the film's device, as for films.
 *
 *   State, from vk_adapt_enable on (48 bytes per pixel and 16 per tile of device memory, nothing before): prev = the sums at the last
 *     close; m2 = sum_j n_j m_j^2 per component in double; per tile tile_n (0 = active, else the count it froze with) and tile_k;
 *     samples_done and steps; the ascending list of the active tiles with the pixels before each.
 *   vk_adapt_enable: ap == NULL keeps moments only and no tile ever freezes; otherwise ap is checked as vk_progress_set_adaptive checks
 *     it, in its words.  VK_ERR_BAD_ARG, the film as it was, once the film has emitted or deposited anything since create or reset;
 *     called again before that it takes the new parameters.  VK_ERR_OOM: the film as it was, nothing kept.  vk_film_reset keeps the
 *     setting and zeroes prev, m2, the tile map, samples_done and steps.
 *   vk_adapt_begin puts `batch` into the regenerating state (vk_regen_*) for the TILE WINDOW: samples [samples_done, samples_done +
 *     n_samples) of every in-image pixel of every active tile, the tile set being the one at the time of the call.  The sequence: active
 *     tiles in ascending tile index t = ty * tiles_x + tx (tile row 0 at the bottom); tw = min(8, W - 8 tx), th = min(8, H - 8 ty); pixel
 *     j < tw * th of a tile is x = 8 tx + j % tw, y = 8 ty + j / tw; P_a = the in-image pixels of the active tiles before the a-th.  Path
 *     q has p = q / n_samples, k = q - p * n_samples, a = the largest index with P_a <= p, j = p - P_a: it is sample samples_done + k of
 *     that pixel, its ray and state vk_film_emit's for that (pixel, sample) bit for bit, its id q.  The run is stepped, culled, read and
 *     finished by vk_regen_step, vk_regen_cull, vk_paths_read and vk_paths_get_info as any regenerating run (six launches a bounce, five
 *     without a top-up).  VK_ERR_BAD_ARG, nothing enqueued, film and batch as they were: a null pointer, a film not enabled, n_samples
 *     == 0, samples_done + n_samples > samples_per_pixel, 2^32 paths or more, a batch of another scene.  With no tile active: VK_OK, and
 *     the run is finished at once.
 *   vk_adapt_close is the caller's statement that every pixel of every active tile has received exactly the samples [samples_done,
 *     samples_done + n_samples) since the last close — by a tile run, by rectangular vk_regen_begin runs, by vk_film_emit and
 *     vk_film_deposit, or a mix.  A wrong statement is the caller's error and is not detected (as emitting a sample twice is not); what
 *     is deposited into a frozen tile never enters its moments, its count or vk_adapt_resolve's image.  On the device, for the pixels
 *     of the active tiles, in this order and without contraction: w = sums - prev; prev = sums; s = (double)w * 2^-26; m2 += s * s /
 *     (double)n_samples.  Then samples_done += n_samples, steps += 1 and, with parameters set, vk_progress_set_adaptive's rule at
 *     (samples_done, steps): a converged tile freezes there.  The list is rebuilt on the device; one record of counts comes back.  With
 *     no tile active a close is VK_OK: samples_done and steps advance, no tile changes.  info may be NULL.  VK_ERR_BAD_ARG, the film
 *     unchanged: not enabled, n_samples == 0, samples_done + n_samples > samples_per_pixel.  Call it with no run of this film under way.
 *   vk_adapt_resolve: vk_film_resolve's arithmetic on the sums of the last close, each pixel divided by its tile's own count (tile_n, or
 *     samples_done for an active tile).  VK_ERR_BAD_ARG while samples_done == 0.
 *   vk_adapt_stderr: vk_progress_stderr's expression with each tile's own N and k, f32 [height][width][3], y = 0 the bottom row.
 *     VK_ERR_BAD_ARG while steps < 2.
 *   vk_adapt_tile_samples: the layout and meaning of vk_progress_tile_samples (out and info may each be NULL).
 *   Contract, with no roulette rule and no cull, where the film's own contract holds:
 *     1. moments: when the n_samples of the closes are the n_samples of the steps of a vk_progress handle with VK_PROGRESS_STDERR, the
 *        same scene, camera and parameters and clamped_samples == 0, prev and m2 are that handle's running sums and moments and
 *        vk_adapt_stderr is its vk_progress_stderr, bit for bit — whatever routes, capacities and slicing carried the samples;
 *     2. decisions: with the same vk_adaptive_params the tile map after every close is the handle's after the same step and
 *        vk_adapt_resolve that step's image, bit for bit: every pixel is vk_render's at its tile's count;
 *     3. schedule: a tile run's vk_paths_read after every bounce is a function of the sequence above, the capacity and the paths'
 *        lifetimes alone.                                                                                                         */
typedef struct vk_adapt_info {           /* 32 bytes */
    uint32_t samples_done, steps;
    uint32_t tiles_total, tiles_active;
    uint64_t pixels_active;              /* in-image pixels of the active tiles */
    uint64_t samples_rendered;           /* pixel-samples the closes have counted, summed over the tiles */
} vk_adapt_info;
int vk_adapt_enable(vk_film *film, const vk_adaptive_params *ap);
int vk_adapt_begin(vk_film *film, vk_paths *batch, uint32_t n_samples);
int vk_adapt_close(vk_film *film, uint32_t n_samples, vk_adapt_info *info);
int vk_adapt_resolve(vk_film *film, float *rgb_out);
int vk_adapt_stderr(vk_film *film, float *out);
int vk_adapt_tile_samples(vk_film *film, uint32_t *out, vk_adaptive_info *info);

/* ---- reconstruction filters: a finished path batch splatted into a filtered frame (additive symbols of ABI 7) -----------------------
 * replaces: nothing (the reference's frame is box-filtered: a sample of pixel (x, y) adds to pixel (x, y) only, and vk_render,
 * vk_progress_* and vk_film_deposit keep doing that).  An accumulator holds, per pixel, four 64-bit two's-complement sums in 2^-26
 * units — r, g, b and the filter weight, interleaved, width * height * 32 bytes — and one record of counters (8 KiB), on the scene's device
 * (devices[0] of a multi-device scene).  All work is on the null stream there; no function takes a stream.  A batch goes in as it goes
 * into a film: finished (nothing live), once per begin or emit — a flag of its own next to the film's, cleared where that one is
 * cleared, so that one batch may go once into a film and once into an accumulator, in either order.
 *
 * The definition, operation by operation.  Everything is f32, unfused, in the order written.
 *   1. Which results.  Every started id is a candidate.  One whose status is VK_SHADE_MISS, VK_SHADE_ENDED or VK_PATHS_CULLED and whose
 *      position (2.) lies in the frame is PLACED; every other candidate counts in `skipped`.  A placed one whose acc has a non-finite
 *      component counts in `dropped`; the rest count in `deposited`.
 *   2. Position.  positions == NULL: the anchor is ix = state.pixel % width, iy = state.pixel / width; state.pixel >= width * height is
 *      not placed; fx and fy are draws 0 and 1 (gen::<f32>(), vk_math.h gen_f32) of the stream of (state.seed, state.pixel,
 *      state.sample) — for a film's camera path exactly the jitter its ray was generated with.  positions != NULL: host memory, 2 *
 *      started floats (px, py) per id, frame coordinates in pixels, y up, pixel (i, j) covering [i, i + 1) x [j, j + 1): ix =
 *      floor(px), fx = px - floor(px), the same in y; a non-finite coordinate, floor(px) < 0 or >= width, floor(py) < 0 or >= height
 *      is not placed (-0.0 is pixel 0).  state.pixel is not read then.
 *   3. Weights.  Per axis, for k = -2 .. 2: d = (fx - 0.5f) - (float)k, the sample's distance from the centre of pixel ix + k; it is in
 *      support iff -radius <= d < radius (half-open: BOX at 0.5 gives each sample to exactly one pixel, fx = 0 included).  With a =
 *      |d| and inv_r = 1.0f / radius:
 *        BOX       w1 = 1
 *        TENT      w1 = 1 - a * inv_r
 *        MITCHELL  t = a * (2 * inv_r);  t < 1: w1 = ((p3 * t + p2) * t) * t + p0;  else w1 = ((q3 * t + q2) * t + q1) * t + q0, with
 *                  p3 = ((12 - 9 * b) - 6 * c) / 6, p2 = ((-18 + 12 * b) + 6 * c) / 6, p0 = (6 - 2 * b) / 6, q3 = (-b - 6 * c) / 6,
 *                  q2 = (6 * b + 30 * c) / 6, q1 = (-12 * b - 48 * c) / 6, q0 = (8 * b + 24 * c) / 6, computed once by the host.
 *      The weight on pixel (ix + kx, iy + ky) is w = wx * wy.  Pairs in support on both axes whose pixel lies inside the frame count in
 *      `contributions`; footprint pixels outside the frame get nothing (the weight sum makes up for it at the resolve).
 *   4. Sums.  With F = ceil(2 * radius)^2 and clamp = min(1e10, 1.3e11 / (float)(samples_per_pixel * F)): a sample whose largest
 *      |component| exceeds 31.999 has its components clamped to +-clamp first and counts in `clamped` if that largest exceeds the clamp
 *      — the film's rule, and at radius 0.5 (F = 1) the film's clamp; F keeps samples_per_pixel * F samples a pixel from wrapping
 *      the 64-bit sums.  Then per footprint pixel: trunc((w * a_c) * 2^26) is added to the sum of c = r, g, b and trunc(w * 2^26) to
 *      the weight sum (|w| <= 1 for all three filters).
 *   5. Resolve.  rgb_c = w_sum > 0 ? ((float)c_sum * 2^-26) / ((float)w_sum * 2^-26) : 0 — a pixel that received nothing, or negative
 *      lobes only, is black —, in vk_render's f32 layout (y = 0 the bottom row).  The call waits; the sums stay.
 * Contract: the sums and counters are a function of the set of deposited results alone — not of windows, batch sizes, order or the
 * kernel's form —, equal tests/splat_ref.py's numpy restatement bit for bit, and with BOX at radius 0.5 the colour sums are
 * vk_film_deposit's, the weight sum is 2^26 per deposited sample and the resolve is vk_film_resolve's at that count: a film's camera
 * paths give vk_render's frame.
 *
 *   vk_splat_default_params: MITCHELL, radius 2, b = c = 1/3.
 *   vk_splat_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, width * height > 2^26, samples_per_pixel outside 1..2^26,
 *     an unknown filter, a radius that is not finite or outside [0.5, 2], MITCHELL with b or c not finite or outside [0, 1].
 *     VK_ERR_OOM leaves *out untouched.
 *   vk_splat_deposit: VK_ERR_BAD_ARG, nothing enqueued or written: a null accumulator or batch, a batch of another scene, one never
 *     begun, a regenerating one, one with live paths, one already deposited into an accumulator since its last vk_paths_begin /
 *     vk_film_emit.
 *   vk_splat_reset zeroes sums and counters.  vk_splat_get_info waits.  vk_splat_destroy(NULL) does nothing.                       */
enum { VK_SPLAT_BOX = 0, VK_SPLAT_TENT = 1, VK_SPLAT_MITCHELL = 2 };
typedef struct vk_splat vk_splat;        /* opaque */
typedef struct vk_splat_params {         /* 16 bytes */
    uint32_t filter;                     /* VK_SPLAT_* */
    float radius;                        /* in pixels, 0.5 .. 2 */
    float b, c;                          /* MITCHELL's; ignored otherwise */
} vk_splat_params;
typedef struct vk_splat_info {           /* 64 bytes */
    uint32_t width, height, samples_per_pixel, filter;
    uint64_t deposited, dropped, clamped, skipped, deposits, contributions;      /* deposits: accepted vk_splat_deposit calls */
} vk_splat_info;
int vk_splat_default_params(vk_splat_params *out);
int vk_splat_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, const vk_splat_params *sp,
                    vk_splat **out);
int vk_splat_deposit(vk_splat *s, vk_paths *batch, const float *positions);
int vk_splat_resolve(vk_splat *s, float *rgb_out);
int vk_splat_reset(vk_splat *s);
int vk_splat_get_info(vk_splat *s, vk_splat_info *out);
void vk_splat_destroy(vk_splat *s);

/* ---- robust film: bucketed sums and Gini-trimmed means for path batches (additive symbols of ABI 7) --------------------------------
 * replaces: nothing (every other frame is a plain mean, as the reference's is: one firefly — one bright sample — lands in the image at
 * full strength and spoils the error estimate, see vk_progress_stderr).  The answer is median of means: an accumulator keeps K partial
 * sums per pixel instead of one and resolves them with an estimator that drops the outlying buckets only where the buckets disagree
 * (the Gini-weighted form, "G-MoN"); on smooth pixels it stays the plain mean.  The standard error of the kept bucket means is a
 * robust stderr3 for vk_denoise and vk_temporal_accumulate.
 *
 * State.  Per pixel and bucket b < K four 64-bit two's-complement words — the sums of r, g, b in 2^-26 units and a count —, width *
 * height * K * 32 bytes, and one record of counters (8 KiB), on the scene's device (devices[0] of a multi-device scene).  All work is on
 * the null stream there; no function takes a stream.  A batch goes in as it goes into a film: finished (nothing live), once per begin
 * or emit — a flag of its own next to the film's and the splat accumulator's, cleared where those are cleared, so that one batch may go
 * once each into a film, a splat accumulator and a robust accumulator, in any order.
 *
 * Deposit.  Every started id is a candidate.  Placement, drop, skip and clamp are vk_film_deposit's rule exactly, with clamp = min(1e10,
 * 1.3e11 / (float)samples_per_pixel): a candidate whose status is VK_SHADE_MISS, VK_SHADE_ENDED or VK_PATHS_CULLED and whose
 * state.pixel < width * height is placed, every other one counts in `skipped` and touches nothing; a placed one whose acc has a
 * non-finite component counts in `dropped`, the rest in `deposited`; a sample whose largest |component| exceeds 31.999 has its
 * components clamped to +-clamp first and counts in `clamped` if that largest exceeds the clamp; the fixed value of a component is
 * trunc(a_c * 2^26).  The target is pixel state.pixel, bucket b = state.sample % K.  A deposited result adds its three fixed values to
 * the sums and 1 to the count; a dropped one adds 1 to the count only (the reference divides by every sample, main.rs:192-197).
 *
 * Resolve, per pixel.  Everything is f32, unfused, in the order written.
 *   1. j = the number of buckets with count > 0.  j = 0: rgb = 0 and stderr = 0.
 *   2. Per non-empty bucket: m_c = ((float)sum_c * 2^-26) / (float)count, Y = (0.2126f * m_r + 0.7152f * m_g) + 0.0722f * m_b.
 *   3. The non-empty buckets are ordered by Y ascending, ties by bucket index ascending: Y_1 .. Y_j.
 *   4. tmax = (j - 2) / 2 in integer division, 0 for j < 2.  The trim t per side:
 *        MEAN  t = 0.
 *        TRIM  t = min(trim, tmax).
 *        GINI  accumulated ascending from 0: num = sum_i (float)(2i - j - 1) * Y_i and s = sum_i Y_i;
 *              G = (Y_1 >= 0 && s > 0) ? num / ((float)j * s) : 0;  h = (G * (float)j) * 0.5f;
 *              t = min(h >= 1 ? (uint32_t)floorf(h) : 0, tmax)  (an h below 1 — a G that rounding left below 0 included — trims nothing).
 *   5. The kept set S is the ordered buckets t + 1 .. j - t; q = j - 2t.
 *   6. rgb_c = ((float)(sum over S of sum_c) * 2^-26) / (float)(sum over S of count); both are integer sums (64-bit, wrapping).
 *   7. q >= 2, in kept order, accumulated ascending from 0: M_c = (sum over S of m_c) / (float)q, e_c = sum over S of (m_c - M_c) *
 *      (m_c - M_c), stderr_c = sqrtf(e_c / (float)(q * (q - 1))).  Otherwise stderr_c = 0.
 * The output is in vk_render's f32 layout (y = 0 the bottom row).  The sums stay; the call waits.  `how` (NULL: create's) lets one
 * accumulator be resolved several ways: its mode and, in TRIM mode, its trim are taken; how->buckets must be the accumulator's or 0.
 *
 * Contract.  (1) The state is a function of the set of deposited results alone — not of windows, batch sizes or order — and equals
 * tests/robust_ref.py's numpy restatement bit for bit.  (2) Summed over the buckets the colour sums are vk_film_deposit's and the
 * counters are the film's.  (3) MEAN on a frame in which every (pixel, sample) below samples_per_pixel went in exactly once is
 * vk_film_resolve(film, samples_per_pixel): vk_render's frame bit for bit wherever the film's contract holds.  (4) The TRIM and GINI
 * images and the stderr equal the restatement bit for bit.
 * What this is not.  TRIM and GINI are biased towards dark where a pixel's buckets legitimately disagree (a light seen by few samples);
 * the bias is bounded by the trimmed share, 2t / j of the buckets.  Buckets of unequal count are ranked as equals.  stderr3 is 0 where
 * fewer than two buckets are kept.  A regenerating batch is refused (its results are not kept), as vk_splat_deposit refuses it.
 *
 *   vk_robust_default_params: 8 buckets, GINI, trim 0.
 *   vk_robust_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, buckets outside 2..16, width * height * buckets > 2^27,
 *     samples_per_pixel outside 1..2^26, an unknown mode, a non-zero _pad.  trim is read in TRIM mode only.  VK_ERR_OOM leaves *out
 *     untouched.
 *   vk_robust_deposit: VK_ERR_BAD_ARG, nothing enqueued or written: a null accumulator or batch, a batch of another scene, one never
 *     begun, a regenerating one, one with live paths, one already deposited into a robust accumulator since its last vk_paths_begin /
 *     vk_film_emit.
 *   vk_robust_resolve: VK_ERR_BAD_ARG for a null accumulator or rgb_out, a `how` of other buckets, of an unknown mode or with a
 *     non-zero _pad.  stderr3_out may be NULL.
 *   vk_robust_reset zeroes sums and counters.  vk_robust_get_info waits.  vk_robust_destroy(NULL) does nothing.                    */
enum { VK_ROBUST_MEAN = 0, VK_ROBUST_TRIM = 1, VK_ROBUST_GINI = 2 };
typedef struct vk_robust vk_robust;      /* opaque */
typedef struct vk_robust_params {        /* 16 bytes */
    uint32_t buckets;                    /* K, 2 .. 16 */
    uint32_t mode;                       /* VK_ROBUST_* */
    uint32_t trim;                       /* TRIM's buckets per side; ignored otherwise */
    uint32_t _pad;                       /* 0 */
} vk_robust_params;
typedef struct vk_robust_info {          /* 64 bytes */
    uint32_t width, height, samples_per_pixel, buckets;
    uint64_t deposited, dropped, clamped, skipped, deposits, _reserved;          /* deposits: accepted vk_robust_deposit calls */
} vk_robust_info;
int vk_robust_default_params(vk_robust_params *out);
int vk_robust_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, const vk_robust_params *rp,
                     vk_robust **out);
int vk_robust_deposit(vk_robust *s, vk_paths *batch);
int vk_robust_resolve(vk_robust *s, const vk_robust_params *how, float *rgb_out, float *stderr3_out);
int vk_robust_reset(vk_robust *s);
int vk_robust_get_info(vk_robust *s, vk_robust_info *out);
void vk_robust_destroy(vk_robust *s);

/* ---- light-path layers: a path batch's frame split by bounce history (additive symbols of ABI 7) ---------------------------------
 * replaces: a host loop around vk_trace_rays and vk_shade_hits kept only to see each bounce's status and lobe (336 bytes per path and
 * bounce over the bus, and in a scene with a medium not the same sample).  Every other accumulator takes a finished path's final acc
 * and nothing else; this one also knows what the path did: emission seen directly, sky, direct against indirect light, a diffuse
 * against a specular or glass first bounce, a medium's in-scatter, one light's contribution.  In this integrator a path has ONE
 * contribution — it ends on an emitter or on the sky — so the class of a path is the class of its whole acc, and layers partition the
 * film's integer sums exactly.
 *
 * Tags.  A tracker keeps two 32-bit words per path id, `sig` and `term`, in a table of `capacity` entries.  A bounce's event code (4
 * bits) is a function of its vk_shaded record's status and lobe as the compaction's count pass leaves them (a roulette cull shows as
 * VK_PATHS_CULLED and keeps its lobe):
 *     VK_SHADE_MISS                          1   VK_LPE_SKY
 *     VK_SHADE_BAD_HIT                      15   VK_LPE_BAD
 *     any other status, lobe 0 .. 5   2 + lobe   2 Lambertian, 3 Metal, 4 Dielectric, 5 DiffuseLight (VK_LPE_EMIT), 6 Isotropic,
 *                                                7 SpecDiffuse
 *     any other status, any other lobe      14   VK_LPE_OTHER
 * and 0 means "no bounce recorded".  For bounce number b of the batch (vk_paths_info.bounces before the bounce; the first is 0) every
 * item of the bounce has its tag updated: b == 0: sig = code | code << 28; otherwise nibble b becomes the code if b < 7, and nibble 7
 * becomes the code whatever b is.  term = the hit record's material where hit == 1, else 0xFFFFFFFF.  So nibbles 0 .. 6 are the first
 * seven bounces, and nibble 7 and term describe the last bounce the path took part in.  A started id no bounce has touched since the
 * tracker was bound has sig 0 and term 0.
 *
 * vk_lpe_step is vk_paths_step with one more launch per bounce (kernel_launches counts six a bounce): lpe_record_kernel, behind the
 * compaction, on the bounce's records, hits and ids.  It launches what vk_paths_step launches, the handle's roulette rule included:
 * after every bounce vk_paths_read and vk_paths_results are byte for byte vk_paths_step's.  A step on a batch whose bounces == 0 BINDS
 * the tracker to that batch and that begin (vk_paths_begin or vk_film_emit); every later call checks the binding.  vk_paths_cull
 * between steps is allowed: a path culled by it keeps the tag of its last recorded bounce.  vk_lpe_tags returns the tags of the
 * started ids (either pointer may be NULL) and waits.
 *
 * Rules and layers.  A result — status, state.depth and the id's tag — matches a rule when (sig & sig_mask) == sig_value, and
 * status_mask >> status & 1, and depth_min <= state.depth <= depth_max, and emitter == 0xFFFFFFFF or emitter == term.  The first
 * matching rule gives the layer; without one the layer is rest_layer.
 *
 * State.  Per pixel and layer four 64-bit two's-complement words — the sums of r, g, b in 2^-26 units and a count —, width * height *
 * n_layers * 32 bytes, 8 bytes per id of the tag table and one record of counters (8 KiB), on the scene's device (devices[0] of a
 * multi-device scene).  All work is on the null stream there; no function takes a stream.
 *
 * Deposit.  Placement, drop, skip, clamp and the counters are vk_film_deposit's rule exactly, as vk_robust_deposit restates it; the
 * target cell is (state.pixel, layer).  A deposited result adds its three fixed values and 1 to the count, a dropped one 1 to the
 * count only.  The batch carries a flag of its own next to the film's, the splat accumulator's and the robust accumulator's, cleared
 * where those are: one batch goes once each into a film, a splat, a robust and a layer accumulator, in any order.
 *
 * Resolve.  rgb_c = ((float)sum_c * 2^-26) / (float)n per channel, in vk_render's f32 layout (y = 0 the bottom row); share_out (may be
 * NULL, one float per pixel) = (float)count / (float)n.  layer == VK_LPE_ALL adds the layers' integer sums first (64-bit, wrapping).
 *
 * Contract.  (1) vk_lpe_tags equals the tags tests/lpe_ref.py derives from every bounce's records of the CPU emulation, bit for bit.
 * (2) The state is a function of the set of deposited results and their tags alone and equals that restatement; summed over the layers
 * the colour sums are vk_film_deposit's, the counts the samples, the counters the film's.  (3) VK_LPE_ALL on a frame in which every
 * (pixel, sample) below n went in once is vk_film_resolve(film, n): vk_render's frame bit for bit wherever the film's contract holds.
 * What this is not.  Regenerating runs are refused: their results are not kept and their ids are not bounded by a capacity.  A
 * multi-device scene uses devices[0] only.  No function takes a stream.  Nothing the integrator samples changes: a layer is a
 * classification of the samples vk_paths_step draws, not a different estimator (light groups split by the emitter that was HIT).
 *
 *   vk_lpe_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, n_layers outside 1..16, width * height * n_layers > 2^27,
 *     samples_per_pixel outside 1..2^26, capacity outside 1..2^24, rest_layer >= n_layers, n_rules > 32, n_rules > 0 with null rules, a
 *     non-zero _pad, and a rule with sig_value & ~sig_mask non-zero, a status_mask that is 0 or has a bit other than MISS, ENDED and
 *     CULLED (1 << status), depth_min > depth_max, layer >= n_layers or a non-zero _pad.  The rules are copied.  VK_ERR_OOM leaves *out
 *     untouched.
 *   vk_lpe_step: VK_ERR_BAD_ARG, nothing enqueued: a null pointer, a batch of another scene, one never begun, a regenerating one,
 *     started > capacity, max_bounces == 0, a batch with bounces > 0 the tracker is not bound to, or whose bounces differ from the
 *     bounces the tracker recorded (a vk_paths_step in between).
 *   vk_lpe_tags: refused for a batch the tracker is not bound to.
 *   vk_lpe_deposit: VK_ERR_BAD_ARG, nothing enqueued or written: what vk_robust_deposit refuses (the flag being this accumulator's
 *     kind), started > capacity, a batch the tracker is not bound to, a batch whose bounces were not all recorded.
 *   vk_lpe_resolve: VK_ERR_BAD_ARG for a null tracker or rgb_out, a layer that is neither below n_layers nor VK_LPE_ALL, n == 0.
 *   vk_lpe_reset zeroes sums and counters (not the tags or the binding).  vk_lpe_get_info waits.  vk_lpe_destroy(NULL) does nothing.
 *   Destroy a tracker before its scene.                                                                                              */
enum { VK_LPE_SKY = 1, VK_LPE_EMIT = 5, VK_LPE_OTHER = 14, VK_LPE_BAD = 15 };
#define VK_LPE_ALL 0xFFFFFFFFu
typedef struct vk_lpe vk_lpe;            /* opaque */
typedef struct vk_lpe_rule {             /* 32 bytes */
    uint32_t sig_mask, sig_value;        /* (sig & sig_mask) == sig_value */
    uint32_t status_mask;                /* bit VK_SHADE_MISS, VK_SHADE_ENDED, VK_PATHS_CULLED */
    uint32_t depth_min, depth_max;       /* of state.depth, inclusive */
    uint32_t emitter;                    /* 0xFFFFFFFF: any; else term must equal it */
    uint32_t layer;
    uint32_t _pad;                       /* 0 */
} vk_lpe_rule;
typedef struct vk_lpe_params {           /* 24 bytes */
    uint32_t n_layers;                   /* 1 .. 16 */
    uint32_t rest_layer;
    uint32_t n_rules;                    /* 0 .. 32 */
    uint32_t _pad;                       /* 0 */
    const vk_lpe_rule *rules;
} vk_lpe_params;
typedef struct vk_lpe_info {             /* 80 bytes */
    uint32_t width, height, samples_per_pixel, n_layers, rest_layer, n_rules;
    uint64_t capacity;
    uint64_t deposited, dropped, clamped, skipped, deposits, recorded;      /* deposits: accepted calls; recorded: path-bounces */
} vk_lpe_info;
int vk_lpe_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t samples_per_pixel, uint64_t capacity,
                  const vk_lpe_params *lp, vk_lpe **out);
int vk_lpe_step(vk_lpe *s, vk_paths *batch, uint32_t max_bounces, vk_paths_step_info *info);
int vk_lpe_tags(vk_lpe *s, vk_paths *batch, uint32_t *sig, uint32_t *term);
int vk_lpe_deposit(vk_lpe *s, vk_paths *batch);
int vk_lpe_resolve(vk_lpe *s, uint32_t layer, uint32_t n, float *rgb_out, float *share_out);
int vk_lpe_reset(vk_lpe *s);
int vk_lpe_get_info(vk_lpe *s, vk_lpe_info *out);
void vk_lpe_destroy(vk_lpe *s);

/* ---- display transform: auto-exposure, tone curves and sRGB on the device (additive symbols of ABI 7) ------------------------------
 * replaces: nothing (Vec3::to_color — square-root gamma, clamp at 0.999, times 256: vk_to_color_device, VK_OUTPUT_RGB8 — stays what it
 * is and is this transform's identity setting).  What a frame of a path tracer needs before a screen can show it: an exposure metered
 * from the frame itself, stable over an animation; a tone curve with a shoulder; a real transfer function, with dither.
 *
 * State.  A handle for one width x height on the scene's device (devices[0] of a multi-device scene): a frame (f32, vk_render's layout,
 * y = 0 the bottom row), a luminance histogram of 640 bins with four counters, the metered exposure, and the two tables of the table
 * transfers.  All work is on the null stream there; no function takes a stream.  vk_tone_load_device and vk_tone_encode_device are
 * ENQUEUED on the null stream: work the caller issued earlier on the null stream or on a blocking stream is ordered before them, and
 * the encoded bytes are ready when the null stream is; a caller with a non-blocking stream synchronises first (and waits for the null
 * stream afterwards).  Every other call waits.
 *
 * Definitions.  Everything is integers and f32 / f64 basic arithmetic, unfused, in the order written.
 * Luminance.  Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b, the robust film's.
 * Histogram.  640 bins of u32 — 40 octaves, 16 per octave, taken from the float's own bits — and four 64-bit counters.  Per pixel, in this
 *   order: a pixel with a non-finite component counts in `nonfinite`; else one with Y < 2^-20 (negative and zero included) in `below`;
 *   else one with Y >= 2^20 in `above`; else it counts in bin (f32_bits(Y) >> 19) - (f32_bits(2^-20f) >> 19) and in `binned`.  All
 *   integers: the result depends on neither the launch shape nor the kernel's form.
 * Exposure (vk_tone_solve: f64 basic operations only, no libm call, built without contraction).
 *   1. N = the sum of the bins.  N = 0 (or no weight in step 3): the info carries VK_TONE_METER_EMPTY, log2_target = log2_used = the
 *      previous meter's log2_used (clamped as in step 5) with the exposure of step 6, or, without a previous one, 0 and the exposure
 *      1.0f; an empty meter is not a previous meter for the next.
 *   2. lo = (double)low_fraction * N, hi = (1.0 - (double)high_fraction) * N.
 *   3. Ascending over the bins, c the count before bin b: w_b = max(0, min(c + bins[b], hi) - max(c, lo)); l_b = -20 + (b + 0.5) / 16;
 *      S += w_b * l_b; W += w_b.
 *   4. log2_target = S / W.
 *   5. log2_used = prev ? prev + (double)blend * (log2_target - prev) : log2_target, then clamped to [min_log2, max_log2].
 *   6. exposure = (float)((double)key * pexp2(-log2_used)), pexp2(x) = ldexp(1 + (x - floor(x)), (int)floor(x)).
 *   l_b and pexp2 are the piecewise-linear log and exp the float format gives for free: each is within 0.0861 octave of the true log2 /
 *   exp2, and a bin's centre within half a bin (1/32 octave) of its members.  The metered exposure therefore puts the trimmed
 *   geometric-mean luminance of the frame within 0.21 octave of `key`.
 *   vk_tone_default_meter_params: key 0.18, low_fraction 0.10, high_fraction 0.02, blend 1, min_log2 -16, max_log2 16.
 * Encode, per pixel and component, f32.  E = params.exposure * (VK_TONE_USE_METERED ? the metered exposure : 1.0f), once on the host.
 *   1. x = rgb_c * E.
 *   2. The curve.  VK_TONE_CLAMP: y = x untouched (NaN and negatives go on to the transfer as they are).  Every other curve first
 *      sanitises: s = x > 0 ? (x < 1048576.0f ? x : 1048576.0f) : 0.0f (NaN becomes 0, +inf 2^20).
 *        VK_TONE_REINHARD (on luminance; w2 = white * white on the host): Ys = Y(s_r, s_g, s_b); k = (1 + Ys / w2) / (1 + Ys); y_c = s_c * k.
 *        VK_TONE_HABLE (per channel): h(v) = ((v * (A * v + C * B) + D * E_) / (v * (A * v + B) + D * F)) - E_ / F with A .15f, B .5f,
 *          C .1f, D .2f, E_ .02f, F .3f; y = h(2.0f * s) / h(white), h(white) computed on the host in f32 by the same function.
 *        VK_TONE_ACES (Narkowicz's fit, per channel): y = (s * (2.51f * s + 0.03f)) / (s * (2.43f * s + 0.59f) + 0.14f).
 *   3. The transfer.  VK_TONE_TRANSFER_REFERENCE: Vec3::to_color's component — sqrtf, the hand-written clamp that NaN falls through,
 *      256.0f *, the saturating cast.  VK_TONE_TRANSFER_SRGB and VK_TONE_TRANSFER_GAMMA22: a table of 510 ascending floats H[j], j = 1 ..
 *      510, H[j] the smallest f32 not below inv(j / 510), inv the inverse sRGB encoding (c <= 0.04045 ? c / 12.92 : ((c + 0.055) /
 *      1.055)^2.4) or c^2.2, evaluated in f64 on the host.  Undithered: code = #{k in 1 .. 255 : y >= H[2k - 1]} (round to nearest).
 *      Dithered (VK_TONE_DITHER): base = #{k in 1 .. 255 : y >= H[2k]}; base = 255 stays 255; otherwise lo = base ? H[2 base] : 0, hi =
 *      H[2 base + 2], fr = (y - lo) / (hi - lo), u = the next gen_f32 of rng_for_stream(params.seed, pixel) (vk_math.h; pixel = the
 *      input index y * width + x, y up; three draws per pixel in r, g, b order, drawn whether used or not), code = base + (u < fr).
 *   4. The byte goes to row height - 1 - y: width * height * 3 bytes, row 0 the TOP, as VK_OUTPUT_RGB8.
 *   vk_tone_default_params: VK_TONE_ACES, VK_TONE_TRANSFER_SRGB, VK_TONE_USE_METERED, exposure 1, white 11.2, seed 0.
 *
 * Contract.  (1) Histogram and counters equal tests/tone_ref.py's numpy restatement exactly, in both kernel forms.  (2) vk_tone_meter's
 * info is vk_tone_solve's on that histogram (vk_tone_meter calls it; below, above and nonfinite are the meter's own, 0 from
 * vk_tone_solve), bit for bit the Python restatement's.  (3) VK_TONE_CLAMP + VK_TONE_TRANSFER_REFERENCE with E = 1.0f gives
 * vk_to_color_device's bytes — NaN, +-inf, -0 and negatives included —, hence vk_render's VK_OUTPUT_RGB8 frame.  (4) Every other
 * combination equals the restatement bit for bit given the library's own table (vk_debug_tone_table), and the host build of the
 * per-pixel code.  (5) The table is strictly increasing, each entry not below the f64 value and within one f32 ulp of it.  (6) Against
 * the f64 closed form round(255 * OETF(curve(E * x))) no component is off by more than one code, and at most 1e-4 of them by one.
 * What this is not.  No bloom or glare, no white balance or grading, no 16-bit or float output, no metering weights; a multi-device
 * scene's frame is its devices[0]'s; the frame comes from the caller's buffer.  Glare is a stage of its own in front of this one:
 * vk_glare_* below, whose output vk_tone_load / vk_tone_load_device take.
 *
 *   vk_tone_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, width * height > 2^27.  VK_ERR_OOM leaves *out untouched.
 *   vk_tone_load / vk_tone_load_device: width * height * 3 floats from the host (through the staging path of the host-pointer calls; waits)
 *     or from memory of the handle's device (enqueued).  VK_ERR_BAD_ARG for a null pointer.
 *   vk_tone_solve / vk_tone_meter: VK_ERR_BAD_ARG, nothing enqueued and *out untouched, for a null pointer, a non-zero _pad,
 *     low_fraction or high_fraction negative or non-finite or their sum >= 1, key not finite and positive, blend outside [0, 1], min_log2
 *     or max_log2 non-finite or beyond +-1000, min_log2 > max_log2, a non-finite *prev_log2; vk_tone_meter before a load.
 *   vk_tone_encode / vk_tone_encode_device: VK_ERR_BAD_ARG, nothing enqueued or written, for a null pointer, a non-zero _pad, an unknown
 *     curve, transfer or flag, VK_TONE_DITHER with VK_TONE_TRANSFER_REFERENCE, exposure or white not finite and positive (white = +inf
 *     is allowed with VK_TONE_REINHARD), an encode before a load, VK_TONE_USE_METERED before a meter, a d_rgb8_out that is not 4-byte
 *     aligned.
 *   vk_tone_reset forgets the metered exposure and the frame: the next meter is a first one.  vk_tone_destroy(NULL) does nothing.   */
enum { VK_TONE_CLAMP = 0, VK_TONE_REINHARD = 1, VK_TONE_HABLE = 2, VK_TONE_ACES = 3 };
enum { VK_TONE_TRANSFER_REFERENCE = 0, VK_TONE_TRANSFER_SRGB = 1, VK_TONE_TRANSFER_GAMMA22 = 2 };
enum { VK_TONE_USE_METERED = 1, VK_TONE_DITHER = 2 };            /* vk_tone_params.flags */
enum { VK_TONE_METER_EMPTY = 1 };                                /* vk_tone_meter_info.flags */
typedef struct vk_tone vk_tone;          /* opaque */
typedef struct vk_tone_meter_params {    /* 32 bytes */
    float key;                           /* the luminance the trimmed geometric mean is mapped to */
    float low_fraction, high_fraction;   /* the shares of the binned pixels left out at the dark and at the bright end */
    float blend;                         /* 0 .. 1: how far a later meter moves from the previous log2_used to its own target */
    float min_log2, max_log2;            /* log2_used is clamped to this range */
    uint32_t _pad[2];                    /* 0 */
} vk_tone_meter_params;
typedef struct vk_tone_meter_info {      /* 56 bytes */
    double log2_target, log2_used;
    uint64_t binned, below, above, nonfinite;
    float exposure;
    uint32_t flags;                      /* VK_TONE_METER_* */
} vk_tone_meter_info;
typedef struct vk_tone_params {          /* 32 bytes */
    uint32_t curve;                      /* VK_TONE_CLAMP .. VK_TONE_ACES */
    uint32_t transfer;                   /* VK_TONE_TRANSFER_* */
    uint32_t flags;                      /* VK_TONE_USE_METERED | VK_TONE_DITHER */
    uint32_t _pad;                       /* 0 */
    float exposure;                      /* a factor on top of the metered exposure (or alone) */
    float white;                         /* REINHARD's and HABLE's white point */
    uint64_t seed;                       /* the dither's */
} vk_tone_params;
typedef struct vk_tone_info {            /* 48 bytes */
    uint32_t width, height;
    uint64_t loads, meters, encodes;     /* accepted calls since create */
    float exposure;                      /* the metered exposure; 1.0f before a meter */
    uint32_t metered;                    /* 1 once vk_tone_meter has run since create or reset */
    double log2_used;                    /* the last non-empty meter's; 0 without one */
} vk_tone_info;
int vk_tone_default_meter_params(vk_tone_meter_params *out);
int vk_tone_default_params(vk_tone_params *out);
int vk_tone_create(vk_scene *scene, uint32_t width, uint32_t height, vk_tone **out);
int vk_tone_load(vk_tone *t, const float *rgb);
int vk_tone_load_device(vk_tone *t, const void *d_rgb);
int vk_tone_meter(vk_tone *t, const vk_tone_meter_params *mp, vk_tone_meter_info *out);
int vk_tone_solve(const uint32_t bins[640], const vk_tone_meter_params *mp, const double *prev_log2, vk_tone_meter_info *out);
int vk_tone_encode(vk_tone *t, const vk_tone_params *tp, uint8_t *rgb8_out);
int vk_tone_encode_device(vk_tone *t, const vk_tone_params *tp, void *d_rgb8_out);
int vk_tone_reset(vk_tone *t);
int vk_tone_get_info(vk_tone *t, vk_tone_info *out);
void vk_tone_destroy(vk_tone *t);

/* ---- glare: an energy-conserving bloom stage in front of the display transform (additive symbols of ABI 7) ---------------------------
 * replaces: nothing.  A tone curve clips: a light of radiance 15 and one of radiance 150 encode to the same white patch.  A camera's or
 * an eye's point-spread function leaks a small share of every pixel's energy over a wide neighbourhood, and that halo is what tells the
 * two apart.  vk_glare_apply spreads the share `strength` of a frame's bright part over a pyramid of halved images and takes the same
 * share away where it came from: a float frame in (vk_render's layout, y = 0 the bottom row, 3 floats a pixel), a float frame of the
 * same shape out, which vk_tone_load / vk_tone_load_device take.
 *
 * State.  A handle for one width x height on the scene's device (devices[0] of a multi-device scene): the pyramid's planes B_1 .. B_7
 * and A_1 .. A_7 (about two thirds of a frame) and, after the first host-pointer call, room for a frame in and a frame out.  Nothing is
 * kept between applies.  All work is on the null stream there; no function takes a stream.  vk_glare_apply_device is ordered exactly as
 * vk_tone_encode_device and vk_nlm_filter_device are: ENQUEUED on the null stream: work the caller issued earlier on the null stream or
 * on a blocking stream is ordered before it, and the output is ready when the null stream is; a caller with a non-blocking stream
 * synchronises first (and waits for the null stream afterwards).  d_rgb_out may be d_rgb_in: the last kernel reads its own pixel of
 * the input only, and every other kernel has read the input before it.  vk_glare_apply goes through the staging path of the
 * host-pointer calls and waits; rgb_out may be rgb_in.
 *
 * The operator, exactly.  Everything is f32, unfused, in the order written, with + - *, fmaxf, fminf and compares; one division, and
 * only when threshold > 0.  tests/glare_ref.py restates it in numpy and the two agree bit for bit (a NaN's payload aside).
 *   Sizes.  Level 0 is W x H; level l + 1 is ceil(w_l / 2) x ceil(h_l / 2): a dimension that has reached 1 stays 1.
 *   Weights, on the host in f64 basic arithmetic.  p_0 = 1, p_l = p_{l-1} * (double)falloff; S = p_0 + .. + p_{L-1}, ascending; c_l =
 *     (float)(p_l / S).
 *   Bright part, per pixel of the input I.  s_c = I_c > 0 ? (I_c < 1048576.0f ? I_c : 1048576.0f) : 0.0f (vk_tone's sanitise).  If a
 *     component of I is not finite, B = 0 for the whole pixel.  If threshold == 0, B_c = s_c.  Otherwise Y = (0.2126f * s_r + 0.7152f *
 *     s_g) + 0.0722f * s_b, f = fmaxf(0, Y - threshold) / fmaxf(Y, 1e-20f), B_c = s_c * f.  B_0 = B is never stored.
 *   Down, level l to l + 1: separable, x first.  With clamp(i) = min(max(i, 0), n - 1): d(j) = ((a(clamp(2j - 1)) + 3 * a(clamp(2j))) +
 *     (3 * a(clamp(2j + 1)) + a(clamp(2j + 2)))) * 0.125f, along x on every source row, then the same along y on the result.
 *   Up, level l + 1 to the size of level l: separable, x first.  j = x >> 1, nb = clamp(j - 1) for an even x, clamp(j + 1) for an odd
 *     one; u(x) = (3 * a(j) + a(nb)) * 0.25f, along x, then the same along y.
 *   Pyramid.  B_{l+1} = Down(B_l), l = 0 .. L - 2.  A_{L-1} = c_{L-1} * B_{L-1};  A_l = c_l * B_l + Up(A_{l+1}), l = L - 2 .. 0.
 *   Composite.  out_c = I_c + strength * (A_0,c - B_c).  A component that is not finite stays what it was.  L = 1 or strength = 0 give
 *     out == I as floats (a -0 becomes +0).
 * Away from the border, with threshold 0, the sum of A_0 is the sum of B: what a pixel loses, its neighbourhood gains.  At the border the
 * clamp reflects what would have left the frame.
 * What this is not.  No lens flares, ghosts or diffraction spikes, no chromatic point-spread function, no convolution with a measured
 * kernel: one radially decaying halo whose width doubles per level.
 *
 *   vk_glare_default_params: levels 6, strength 0.15, falloff 1, threshold 0, flags 0.  Touches no device.
 *   vk_glare_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, a size beyond vk_nlm_create's limits (width or height >
 *     65535, width * height * 3 > 2^31).  VK_ERR_OOM leaves *out untouched.
 *   vk_glare_apply / vk_glare_apply_device: VK_ERR_BAD_ARG, nothing enqueued and the output untouched, for a null handle, params, input
 *     or output, levels outside 1..8, strength not finite or outside [0, 1], falloff not finite or <= 0, threshold not finite or < 0,
 *     flags or _pad != 0.
 *   vk_glare_destroy(NULL) does nothing.                                                                                              */
typedef struct vk_glare vk_glare;        /* opaque */
typedef struct vk_glare_params {         /* 24 bytes */
    uint32_t levels;                     /* L: 1..8 */
    float strength;                      /* 0..1: the share of the bright part that is spread */
    float falloff;                       /* > 0: level l has weight proportional to falloff^l */
    float threshold;                     /* >= 0: luminance below which a pixel spreads nothing; 0 = physical glare, everything spreads */
    uint32_t flags;                      /* 0 */
    uint32_t _pad;                       /* 0 */
} vk_glare_params;
typedef struct vk_glare_info {           /* 48 bytes */
    uint32_t width, height;
    uint64_t applies;                    /* accepted calls since create */
    uint32_t last_levels;                /* L of the last apply; 0 before one */
    uint32_t last_form;                  /* VK_GLARE_FORM_PLAIN or VK_GLARE_FORM_FUSED of the last apply; 0 before one */
    uint32_t last_launches;              /* the kernels the last apply launched */
    uint32_t _pad;
    double last_kernel_ms;               /* the device time of the last apply's kernels, first to last; 0 before one (waits for it) */
    uint64_t scratch_bytes;              /* the device memory the handle owns */
} vk_glare_info;
int vk_glare_default_params(vk_glare_params *out);
int vk_glare_create(vk_scene *scene, uint32_t width, uint32_t height, vk_glare **out);
int vk_glare_apply(vk_glare *g, const vk_glare_params *p, const float *rgb_in, float *rgb_out);
int vk_glare_apply_device(vk_glare *g, const vk_glare_params *p, const void *d_rgb_in, void *d_rgb_out);
int vk_glare_get_info(vk_glare *g, vk_glare_info *out);
void vk_glare_destroy(vk_glare *g);

/* ---- point-spread function: aperture glare by FFT convolution with a caller's kernel (additive symbols of ABI 7) --------------------
 * replaces: nothing.  vk_glare is one radially decaying halo; the star, the streaks and the coloured fringe by which a camera or an eye
 * tells one clipped highlight from another are the aperture's point-spread function.  vk_psf_apply convolves the bright part of a float
 * frame with an arbitrary K x K kernel per colour component, up to 1023 pixels wide, spreads the share `strength` of it and takes the
 * same share away where it came from: a float frame in (vk_render's layout, y = 0 the bottom row, 3 floats a pixel), a float frame of
 * the same shape out, which vk_tone_load / vk_tone_load_device take.  In the pipeline it sits between vk_glare and vk_tone.
 *
 * State.  A handle for one width x height and kernels up to kmax on the scene's device (devices[0] of a multi-device scene): three
 * planes F and three planes G of Px x Py complex f32 at kmax's padded size (8 bytes a value), the two twiddle tables, the normalised
 * kernel, and, after the first call that needs them, room for a frame in and a frame out of the host-pointer call and a copy of the
 * input of an in-place apply.  vk_psf_load keeps the kernel's transform G until the next load or vk_psf_reset; nothing else is kept
 * between applies.  All work is on the null stream there; no function takes a stream.  vk_psf_apply_device is ordered exactly as
 * vk_glare_apply_device is: ENQUEUED on the null stream: work the caller issued earlier on the null stream or on a blocking stream is
 * ordered before it, and the output is ready when the null stream is; a caller with a non-blocking stream synchronises first (and waits
 * for the null stream afterwards).  d_rgb_out may be d_rgb_in: the kernel that writes a pixel reads that pixel of the input only (in
 * the LDS form from a copy made first), and every other kernel has read the input before it.  vk_psf_apply goes through the staging path
 * of the host-pointer calls and waits; rgb_out may be rgb_in.  vk_psf_load waits; vk_psf_load_device brings the kernel to the host
 * first (which waits for the null stream), checks and normalises it there, and enqueues the rest.
 *
 * The operator, exactly.  Everything on the device is f32, unfused, in the order written, with + - *, fmaxf, fminf and compares; one
 * division, and only when threshold > 0; no transcendental function.  tests/psf_ref.py restates it in numpy and the two agree bit for
 * bit as floats (-0 equal to +0, a NaN's payload aside).
 *   Kernel.  K x K x 3 floats, K odd, 3 <= K <= 1023, tap (kx, ky) at (ky * K + kx) * 3 + c, y up as the frame, centre at r = (K - 1)
 *     / 2.  Every component finite and >= 0.  S_c = the f64 sum of channel c in ascending index order, > 0; k_c[i] = (float)((double)
 *     k_c[i] / S_c).
 *   Padded size.  Px = the smallest power of two >= W + K - 1, Py the same of H + K - 1; at most 4096 each.  Outside the frame the
 *     source is zero: energy that leaves the frame is lost, and nothing wraps.
 *   Bright part, per pixel of the input I: vk_glare's.  s_c = I_c > 0 ? (I_c < 1048576.0f ? I_c : 1048576.0f) : 0.0f.  If a component
 *     of I is not finite, B = 0 for the whole pixel.  If threshold == 0, B_c = s_c.  Otherwise Y = (0.2126f * s_r + 0.7152f * s_g) +
 *     0.0722f * s_b, f = fmaxf(0, Y - threshold) / fmaxf(Y, 1e-20f), B_c = s_c * f.
 *   Twiddle tables, on the host in f64 with + - * / and sqrt only.  R_q = (c_q, s_q) = (cos, sin)(pi / 2^q): c_1 = 0, s_1 = 1; c_{q+1}
 *     = sqrt((1 + c_q) / 2), s_{q+1} = s_q / (2 * c_{q+1}).  For N = 2^m and k < N / 2: z = (1, 0); for t = 0 .. m - 2 in this order,
 *     if bit t of k is set, z = (z.re * c_q - z.im * s_q, z.re * s_q + z.im * c_q) with q = m - 1 - t.  T[k] = ((float)z.re, (float)(0
 *     - z.im)) = exp(-2 pi i k / N) rounded; T[0] = (1, 0) and T[N/4] = (0, -1) exactly.
 *   1-D transform of a length N = 2^m: radix 2, decimation in time.  a[rev_m(i)] = input[i] (rev_m reverses the m bits).  For s = 1 ..
 *     m, half = 2^(s-1), for every block start b (a multiple of 2^s) and j < half: p = b + j, w = T[j * N / 2^s] (the inverse
 *     transform negates w.im), u = a[p], v = a[p + half]; t.re = v.re * w.re - v.im * w.im, t.im = v.re * w.im + v.im * w.re; a[p] = u
 *     + t, a[p + half] = u - t, componentwise.  Every butterfly does the full multiply.
 *   2-D transform.  Every row along x, then every column along y; the input's imaginary parts are +0.  The inverse is the same with
 *     inverse 1-D transforms, and ends with ONE multiplication by the exact power of two 1 / (Px * Py).
 *   Convolution.  F_c = FFT2(B_c, +0 outside the frame).  G_c = FFT2(k_c placed with its centre at (0, 0), wrapped: tap (kx, ky) at
 *     ((kx - r) mod Px, (ky - r) mod Py)), made once at load.  P = F ⊙ G with the butterfly's multiply, v = F, w = G.  C_c = re(IFFT2(P))
 *     * (1 / (Px * Py)) at the W x H pixels.
 *   Composite.  out_c = I_c + strength * (C_c - B_c).  A component that is not finite stays what it was.  strength = 0 gives out == I
 *     as floats (a -0 becomes +0).
 * vk_psf_star fills a kernel for the CLI and the Python layer; the operator takes any.  In f64, not bit-pinned (it calls libm): with r
 * = (K - 1) / 2, g_c = 1 + chroma * (c - 1) for c = 0, 1, 2, d = sqrt(x^2 + y^2) / g_c for x, y in -r .. r:
 *   v = exp(-d^2 / 2) + [streaks > 0, d > 0, d < r] 0.25 * |cos(streaks / 2 * (atan2(y, x) - rotation))|^sharpness * (1 - d / r)^2 /
 *   (1 + d), each channel then divided by its sum.  `streaks` rays at a spacing of 2 pi / streaks from `rotation` (an even count gives
 *   pairs of opposite rays); with chroma = 0 the three channels are equal.
 * What this is not.  No kernel from an aperture mask, no ghosts or flares, no real-to-complex packing, no sizes that are no power of
 * two, no tiling beyond 4096, no multi-device partition, no clamped or mirrored border.
 *
 *   vk_psf_default_params: strength 0.15, threshold 0, form AUTO, flags and _pad 0.  Touches no device.
 *   vk_psf_star: VK_ERR_BAD_ARG for a null pointer, K even or outside 3..1023, streaks > 64, rotation not finite, sharpness not finite
 *     or < 1, chroma not finite or outside [0, 0.5].  Touches no device.
 *   vk_psf_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, kmax even or outside 3..1023, width + kmax - 1 or height +
 *     kmax - 1 > 4096.  VK_ERR_OOM leaves *out untouched.
 *   vk_psf_load / vk_psf_load_device: VK_ERR_BAD_ARG, the loaded kernel untouched, for a null pointer, K even, outside 3..1023 or >
 *     kmax, a component that is not finite or is negative, a channel whose sum is not > 0.
 *   vk_psf_apply / vk_psf_apply_device: VK_ERR_BAD_ARG, nothing enqueued and the output untouched, for a null handle, params, input or
 *     output, an apply before a load (or after vk_psf_reset), strength not finite or outside [0, 1], threshold not finite or < 0, an
 *     unknown form, flags or _pad != 0.
 *   vk_psf_reset forgets the loaded kernel.  vk_psf_destroy(NULL) does nothing.                                                         */
enum { VK_PSF_FORM_AUTO = 0, VK_PSF_FORM_PLAIN = 1, VK_PSF_FORM_LDS = 2 };
typedef struct vk_psf vk_psf;            /* opaque */
typedef struct vk_psf_params {           /* 20 bytes */
    float strength;                      /* 0..1: the share of the bright part that is spread */
    float threshold;                     /* >= 0: luminance below which a pixel spreads nothing; 0 = everything spreads */
    uint32_t form;                       /* VK_PSF_FORM_*: PLAIN = a launch per butterfly stage over global memory; LDS = whole lines in
                                            LDS, four launches; AUTO = LDS (DESIGN.md "Point-spread function").  All give the same bits. */
    uint32_t flags;                      /* 0 */
    uint32_t _pad;                       /* 0 */
} vk_psf_params;
typedef struct vk_psf_info {             /* 64 bytes */
    uint32_t width, height;
    uint32_t K, Px, Py;                  /* of the loaded kernel; 0 before a load */
    uint32_t kmax;
    uint32_t last_form;                  /* VK_PSF_FORM_PLAIN or VK_PSF_FORM_LDS of the last apply; 0 before one */
    uint32_t last_launches;              /* the kernels the last apply (or, after a load, the load) launched */
    uint64_t loads, applies;             /* accepted calls since create */
    double last_kernel_ms;               /* the device time of the last apply's kernels, first to last; 0 before one (waits for it) */
    uint64_t scratch_bytes;              /* the device memory the handle owns */
} vk_psf_info;
int vk_psf_default_params(vk_psf_params *out);
int vk_psf_star(uint32_t K, uint32_t streaks, float rotation, float sharpness, float chroma, float *out);
int vk_psf_create(vk_scene *scene, uint32_t width, uint32_t height, uint32_t kmax, vk_psf **out);
int vk_psf_load(vk_psf *h, uint32_t K, const float *kernel);
int vk_psf_load_device(vk_psf *h, uint32_t K, const void *d_kernel);
int vk_psf_apply(vk_psf *h, const vk_psf_params *p, const float *rgb_in, float *rgb_out);
int vk_psf_apply_device(vk_psf *h, const vk_psf_params *p, const void *d_rgb_in, void *d_rgb_out);
int vk_psf_reset(vk_psf *h);
int vk_psf_get_info(vk_psf *h, vk_psf_info *out);
void vk_psf_destroy(vk_psf *h);

/* ---- guided upsampling: a low-resolution frame to full size along the edges of full-size AOVs (additive symbols of ABI 7) ------------
 * replaces: nothing.  Render scale: the paths are traced at w x h, the first-hit buffers (vk_render_aov, or vk_render_guides for both
 * sizes) at w x h and at W x H — they cost a small fraction of a frame —, and vk_upsample_apply brings colour and its standard error to
 * W x H by joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele 2007) with the variance carried along.  It takes a colour
 * frame, its stderr3 and first-hit buffers, and gives the colour frame and stderr3 that vk_temporal_accumulate, vk_nlm_load, vk_denoise,
 * vk_glare_apply and vk_tone_load take.  All images are in vk_render's f32 layout, y = 0 the bottom row: colour, stderr3, albedo and
 * normal 3 floats a pixel, depth 1.  Both frames come from the same vk_camera.
 *
 * State.  A handle for one pair of sizes on the scene's device (devices[0] of a multi-device scene): a copy of the loaded low images
 * (13 floats a low pixel), the three prepared planes (12 floats a low pixel), two counters and, after the first host-pointer apply, room
 * for the high guides and the two outputs.  vk_upsample_load packs the low frame into the planes; the caller's buffers are free after
 * it, and a second apply with other parameters needs no reload.  All work is on the null stream there; no function takes a stream.  The
 * _device calls are ordered exactly as vk_glare_apply_device and vk_nlm_load_device are: ENQUEUED on the null stream: work the caller
 * issued earlier on the null stream or on a blocking stream is ordered before it, and the output is ready when the null stream is; a
 * caller with a non-blocking stream synchronises first (and waits for the null stream afterwards).  The host-pointer calls go through
 * the staging path of the host-pointer calls and wait.
 *
 * The operator, exactly.  Everything is f32, unfused, in the order written, with + - * /, sqrtf, fabsf, fmaxf, fminf, floorf and
 * compares.  E(x) = fmaxf(0, 1 - x * 0.125f), squared three times (vk_denoise's).  tests/upsample_ref.py restates it in numpy and the
 * two agree bit for bit (a NaN's payload aside).
 *   Mapping (the reference's frame convention, main.rs:187, as vk_temporal uses it: pixel x covers u in [x / (w - 1), (x + 1) / (w - 1)]).
 *     rx = (float)((double)(w - 1) / (double)(W - 1)) on the host, ry likewise from h and H; px = ((float)X + 0.5f) * rx - 0.5f, py
 *     likewise; x0 = floorf(px), y0 = floorf(py).  sx = (float)((double)(W - 1) / (double)(w - 1)), sy likewise.
 *   Prepare, per low pixel q, at load.  a_c = fmaxf(albedo_c, albedo_floor), or 1 without albedo; I_c = color_c / a_c; V_c = (stderr_c /
 *     a_c)^2, or 0 without stderr3.  q is INVALID if a component of colour, or of stderr3 when given, is not finite.  l2 = (n_x n_x + n_y
 *     n_y) + n_z n_z: l2 < 1e-12f or not finite, or no normal loaded: q has NO NORMAL; otherwise n^ = n / sqrtf(l2).  z = depth if
 *     finite, else +inf.  The planes depend on the floor: an apply with another floor prepares them again from the handle's copy.
 *   Per high pixel P.  n^_P and z_P from the high guides by the same rules.  The depth slope g_x, g_y from depth_hi, in high pixels:
 *     with dl = z_P - z_left and dr = z_right - z_P, where both neighbours are in the image and finite the one smaller in magnitude if
 *     dl * dr > 0 (fminf for positive ones, fmaxf for negative ones) and 0 otherwise; where one is, that difference; else 0; 0 where z_P
 *     is +inf.  (vk_denoise's central difference reads a depth edge next to P as a slope and lets the far side in; this one does not.)
 *   Taps.  ty = y0 - 1 .. y0 + 2 the outer loop, tx = x0 - 1 .. x0 + 2 the inner, ascending; a tap outside the low image or INVALID is
 *     skipped.  kx = fmaxf(0, 1 - fabsf(px - (float)tx) * 0.5f), ky likewise.  w_n = 1 if the normal term is off or neither pixel has a
 *     normal, 0 if exactly one has, otherwise fmaxf(0, (n^_P.x n^_q.x + n^_P.y n^_q.y) + n^_P.z n^_q.z) squared normal_squarings times.
 *     x_z = 0 if the depth term is off or both depths are +inf; the tap is skipped if exactly one is; otherwise fabsf(z_P - z_q) /
 *     (sigma_z * (fabsf(g_x * ux + g_y * uy) + 0.001f * z_P)), ux = ((float)tx - px) * sx, uy = ((float)ty - py) * sy.
 *     wt = ((kx * ky) * w_n) * E(x_z).  In tap order from 0: Wt += wt, J_c += wt * I_c(q), U_c += (wt * wt) * V_c(q).
 *     A term is on when its guide was loaded and is given to apply; one side only switches it off.
 *   Fallback.  Wt < 1e-4f: no consistent tap; the sums are taken again with wt = kx * ky over the same in-image, valid taps (those the
 *     depth term skipped included) and P counts in fallback_pixels.  Still Wt < 1e-4f: every tap was invalid; out = 0, stderr3_out = 0
 *     and P counts in empty_pixels as well.
 *   Finish.  A_c = fmaxf(albedo_hi_c, albedo_floor), or 1 without albedo; out_c = (J_c / Wt) * A_c; stderr3_out_c = (sqrtf(U_c) / Wt) * A_c.
 * Laws (tests/upsample_laws_ref.py).  A constant low frame gives the constant, whatever the guides.  The tent's weights sum to 2 and
 * have zero first moment at any phase, so a low frame affine in (x, y) under flat guides gives that function at (px, py) wherever the
 * 4 x 4 footprint lies inside the low image.
 * What this is not.  Scale 1 is not the identity: the tent spans two low pixels on either side.  stderr3_out is each pixel's marginal
 * error: neighbouring outputs share taps and are correlated, and a downstream vk_denoise will treat them as independent.  Nothing is
 * followed through mirrors or glass, unless the caller passes vk_render_guides' buffers for both sizes.  No temporal upsampling, no
 * non-uniform scale.
 *
 *   vk_upsample_default_params: sigma_z 1, normal_squarings 7, albedo_floor 1e-3, flags 0 (vk_denoise's).  Touches no device.
 *   vk_upsample_create: VK_ERR_BAD_ARG for a null pointer, w or h < 2, w > W or h > H, a high size beyond vk_nlm_create's limits (W or H
 *     > 65535, W * H * 3 > 2^31).  VK_ERR_OOM leaves *out untouched.
 *   vk_upsample_load / vk_upsample_load_device: VK_ERR_BAD_ARG for a null handle or colour; every other image may be null.
 *   vk_upsample_apply / vk_upsample_apply_device: VK_ERR_BAD_ARG, nothing enqueued and the outputs untouched, for a null handle, params
 *     or rgb_out, sigma_z or albedo_floor not finite or not > 0, normal_squarings > 10, flags or _pad != 0, an apply before a load,
 *     albedo_hi given without a loaded albedo or the other way round (demodulating one side only is a wrong image, not an option),
 *     stderr3_out wanted without a loaded stderr3.
 *   vk_upsample_reset forgets the loaded frame.  vk_upsample_destroy(NULL) does nothing.                                              */
typedef struct vk_upsample vk_upsample;  /* opaque */
enum { VK_UPSAMPLE_HAS_STDERR = 1, VK_UPSAMPLE_HAS_ALBEDO = 2, VK_UPSAMPLE_HAS_NORMAL = 4, VK_UPSAMPLE_HAS_DEPTH = 8 };
typedef struct vk_upsample_params {      /* 20 bytes */
    float sigma_z;                       /* > 0: the depth term's width, in units of the slope's prediction plus 0.1 % of the depth */
    uint32_t normal_squarings;           /* 0..10: the normal term is the cosine to the power 2^normal_squarings */
    float albedo_floor;                  /* > 0 */
    uint32_t flags;                      /* 0 */
    uint32_t _pad;                       /* 0 */
} vk_upsample_params;
typedef struct vk_upsample_info {        /* 80 bytes */
    uint32_t width_lo, height_lo, width_hi, height_hi;
    uint32_t loaded;                     /* 1 after a load, 0 after create and reset */
    uint32_t guides;                     /* VK_UPSAMPLE_HAS_* of the loaded low frame */
    uint64_t loads, applies;             /* accepted calls since create */
    uint32_t last_form;                  /* VK_UPSAMPLE_FORM_PLAIN or _TILED of the last apply; 0 before one */
    uint32_t last_launches;              /* the kernels the last load or apply launched (an apply with a new floor: 2) */
    double last_kernel_ms;               /* the device time of the last apply's filter kernel; 0 before one (waits for it) */
    uint64_t scratch_bytes;              /* the device memory the handle owns */
    uint64_t fallback_pixels;            /* of the last apply (waits for it): pixels filtered by the tent alone, the empty ones included */
    uint64_t empty_pixels;               /* of the last apply: pixels without a valid tap */
} vk_upsample_info;
int vk_upsample_default_params(vk_upsample_params *out);
int vk_upsample_create(vk_scene *scene, uint32_t w, uint32_t h, uint32_t W, uint32_t H, vk_upsample **out);
int vk_upsample_load(vk_upsample *u, const float *color_lo, const float *stderr3_lo, const float *albedo_lo, const float *normal_lo,
                     const float *depth_lo);
int vk_upsample_load_device(vk_upsample *u, const void *d_color_lo, const void *d_stderr3_lo, const void *d_albedo_lo,
                            const void *d_normal_lo, const void *d_depth_lo);
int vk_upsample_apply(vk_upsample *u, const vk_upsample_params *p, const float *albedo_hi, const float *normal_hi, const float *depth_hi,
                      float *rgb_out, float *stderr3_out);
int vk_upsample_apply_device(vk_upsample *u, const vk_upsample_params *p, const void *d_albedo_hi, const void *d_normal_hi,
                             const void *d_depth_hi, void *d_rgb_out, void *d_stderr3_out);
int vk_upsample_reset(vk_upsample *u);
int vk_upsample_get_info(vk_upsample *u, vk_upsample_info *out);
void vk_upsample_destroy(vk_upsample *u);

/* ---- non-local means: denoising a frame from its own standard error (additive symbols of ABI 7) -------------------------------------
 * replaces: nothing.  The spatial filter for frames whose first-hit buffers say little (small textured, glass and metal objects): its
 * weights come from the colour image and its variance alone, by variance-cancelling patch distances (Rousselle, Knaus, Zwicker 2012).
 * The stderr3 of vk_progress_stderr, vk_adapt_stderr, vk_robust_resolve or vk_temporal_* goes in with the frame; a filtered frame and
 * its propagated standard error come out, in the shapes vk_denoise and vk_tone_load take.
 *
 * State.  A handle for one width x height on the scene's device (devices[0] of a multi-device scene, on the whole image): a copy of
 * the loaded images and four planes of three floats a pixel (I, V, Vf, a below) that vk_nlm_load fills from it — 84 bytes a pixel —, so
 * that a second vk_nlm_filter with other parameters needs no reload and the caller's buffers may be reused after the load.  The planes
 * are prepared with the albedo_floor of the last filter (1e-3 before one); a filter with another floor prepares them again from the
 * handle's copy first, one more kernel.  All work is on the null stream there; no function takes a stream.  vk_nlm_load_device and
 * vk_nlm_filter_device are ordered exactly as vk_tone_load_device and vk_tone_encode_device are: ENQUEUED on the null stream: work the
 * caller issued earlier on the null stream or on a blocking stream is ordered before them, and the outputs are ready when the null
 * stream is; a caller with a non-blocking stream synchronises first (and waits for the null stream afterwards).  Every other call
 * waits.
 *
 * The filter, exactly.  Everything is f32, unfused, in the order written, with + - * /, sqrtf, fmaxf, fminf (each returns its other
 * argument when one is a NaN) and compares only; tests/nlm_ref.py restates it in numpy and the two agree bit for bit (a NaN's payload
 * aside).  All images are in vk_render's layout (y = 0 the bottom row), 3 floats per pixel.  E(x) = t^8 with t = fmaxf(0, 1 - x *
 * 0.125f), by three squarings: vk_denoise's.
 *   Prepare (vk_nlm_load), per pixel p.  a_c = fmaxf(albedo_c, albedo_floor), or 1 without albedo; I_c = color_c / a_c; s_c = stderr_c /
 *     a_c, V_c = s_c * s_c, per channel (not vk_denoise's luminance variance).  p is INVALID if a component of color or stderr3 is not
 *     finite: it is never a neighbour and never part of a patch, its out is its color and its stderr3_out its stderr3, unchanged.
 *     Vf_c(p) = (sum of k3 * V_c(q)) / (sum of k3) over the 3x3 adjacent pixels q that are in the image and valid, rows bottom to top, x
 *     ascending, k3 = (1 2 1; 2 4 2; 1 2 1), both sums from 0: vk_denoise's Vg, per channel.
 *   Pair term, for valid a and b, kk = k * k (once, on the host).  Per channel d = I_c(a) - I_c(b); num = d * d - alpha * (Vf_c(a) +
 *     fminf(Vf_c(a), Vf_c(b))); den = 1e-10f + kk * (Vf_c(a) + Vf_c(b)).  e(a, b) = ((num_r / den_r) + (num_g / den_g)) + (num_b /
 *     den_b), c(a, b) = 1.  If a or b is outside the image or invalid: e = 0, c = 0.
 *   Filter (vk_nlm_filter), per valid p.  Offsets o = (ox, oy), oy = -R..R outer, ox = -R..R inner, ascending, q = p + o; offsets whose
 *     q is outside the image or invalid are skipped.  The centre offset has w = 1.  For the others, the patch sum, rows first: for j =
 *     -F..F ascending: r = 0, m = 0; for i = -F..F ascending: r += e(p + (i, j), q + (i, j)), m += c(...); then S += r, n += m (S and n
 *     from 0, n an integer).  D = S / (float)(3 * n)  (n >= 1: the pair (p, q) counts).  w = E(fmaxf(0, D)), and w = 0 if D is a NaN.
 *     In offset order from 0: W += w, J_c += w * I_c(q), U_c += (w * w) * V_c(q)  (the unfiltered V).
 *     out_c = (J_c / W) * a_c, stderr3_out_c = (sqrtf(U_c) / W) * a_c.
 *   The row-then-column order is part of the definition: a form that shares row sums between neighbouring pixels agrees bit for bit
 *   with one that does not (the kernel has both: DESIGN.md "Non-local means").
 * What this is not.  No cross-filtering between two half buffers, no feature-buffer terms in the weights, no multi-scale passes.
 *
 *   vk_nlm_default_params: search_radius 7, patch_radius 3, k 0.45, alpha 1, albedo_floor 1e-3, flags 0.  Touches no device.
 *   vk_nlm_create: VK_ERR_BAD_ARG for a null pointer, width or height 0, a size beyond vk_render's limits (width or height > 65535,
 *     width * height * 3 > 2^31).  VK_ERR_OOM leaves *out untouched.
 *   vk_nlm_load / vk_nlm_load_device: color and stderr3 are required (without a variance the filter is meaningless), albedo may be
 *     NULL; from the host (through the staging path of the host-pointer calls; waits) or from memory of the handle's device (enqueued).
 *     VK_ERR_BAD_ARG for a null handle, color or stderr3.
 *   vk_nlm_filter / vk_nlm_filter_device: VK_ERR_BAD_ARG, nothing enqueued and the outputs untouched, for a null handle, params or
 *     rgb_out (stderr3_out may be NULL), search_radius outside 1..10, patch_radius outside 0..3, k not finite or <= 0, alpha not finite
 *     or < 0, albedo_floor not finite or <= 0, flags != 0, a filter before a load.
 *   vk_nlm_reset forgets the frame: the next filter needs a load.  vk_nlm_destroy(NULL) does nothing.                                 */
typedef struct vk_nlm vk_nlm;            /* opaque */
typedef struct vk_nlm_params {           /* 24 bytes */
    uint32_t search_radius;              /* R: 1..10; the window is (2R + 1)^2 offsets */
    uint32_t patch_radius;               /* F: 0..3; a patch is (2F + 1)^2 pixels */
    float k;                             /* the distance's scale: larger smooths more */
    float alpha;                         /* how much of the variance is cancelled from the squared difference */
    float albedo_floor;                  /* > 0: demodulation divides by max(albedo, albedo_floor) */
    uint32_t flags;                      /* 0 */
} vk_nlm_params;
typedef struct vk_nlm_info {             /* 56 bytes */
    uint32_t width, height;
    uint32_t loaded;                     /* 1 between a load and the next reset */
    uint32_t has_albedo;                 /* 1 if the loaded frame came with an albedo */
    uint64_t loads, filters;             /* accepted calls since create */
    uint32_t last_launches;              /* the kernels the last accepted call launched */
    uint32_t last_form;                  /* VK_NLM_FORM_PLAIN or VK_NLM_FORM_TILED of the last filter; 0 before one */
    double last_kernel_ms;               /* the last filter kernel's device time; 0 before one (waits for it) */
    uint64_t scratch_bytes;              /* the device memory the handle owns */
} vk_nlm_info;
int vk_nlm_default_params(vk_nlm_params *out);
int vk_nlm_create(vk_scene *scene, uint32_t width, uint32_t height, vk_nlm **out);
int vk_nlm_load(vk_nlm *h, const float *color, const float *stderr3, const float *albedo);
int vk_nlm_load_device(vk_nlm *h, const void *d_color, const void *d_stderr3, const void *d_albedo);
int vk_nlm_filter(vk_nlm *h, const vk_nlm_params *p, float *rgb_out, float *stderr3_out);
int vk_nlm_filter_device(vk_nlm *h, const vk_nlm_params *p, void *d_rgb_out, void *d_stderr3_out);
int vk_nlm_reset(vk_nlm *h);
int vk_nlm_get_info(vk_nlm *h, vk_nlm_info *out);
void vk_nlm_destroy(vk_nlm *h);

/* ---- denoising a frame from its error estimate and first-hit buffers (additive symbols of ABI 7) ------------------------------------
 * replaces: nothing.  The consumer of vk_progress_stderr and vk_render_aov: an edge-avoiding, variance-guided a-trous wavelet filter
 * (the spatial half of SVGF: one frame, no history) on the device.  All images are in vk_render's f32 layout (y = 0 the bottom row):
 * color, stderr3, albedo, normal and out 3 floats per pixel, depth 1.  color and out are required; each of stderr3, albedo, normal and
 * depth may be NULL, which switches its term off.  out must not overlap an input.  The filter needs a pixel's neighbours: it works on
 * the whole image (no tile partition), on devices[0] of a multi-device scene.
 *
 * The filter, exactly.  Everything is f32, unfused, in the order written, with + - * /, sqrtf, fabsf, fmaxf (which returns its other
 * argument when one is a NaN) and compares only; tests/denoise_ref.py restates it in numpy and the two agree bit for bit (a NaN's
 * payload aside).  E(x) = t^8 with t = fmaxf(0, 1 - x * 0.125f), by three squarings: a compact-support stand-in for exp(-x).
 *   Prepare, per pixel p.  a_c = fmaxf(albedo_c, albedo_floor), or 1 without albedo; I_c = color_c / a_c.  With stderr3: s_c = stderr_c /
 *     a_c, sd = (0.2126f*s_r + 0.7152f*s_g) + 0.0722f*s_b, V = sd * sd (the components taken as fully correlated: an upper bound, on
 *     purpose); without: V = 0.  p is INVALID if a component of color (or of stderr3, when given) is not finite: it is never a
 *     neighbour and its out is its color, unchanged.  Normal: l2 = (n_x*n_x + n_y*n_y) + n_z*n_z; l2 < 1e-12f or not finite (a miss, a
 *     medium hit): p has NO NORMAL; else n^ = n / sqrtf(l2).  Depth: z = depth if finite, else +inf.  Depth slope: g_x = (z(x+1) -
 *     z(x-1)) * 0.5f where both neighbours are in the image and finite, else the one-sided difference z(x+1) - z or z - z(x-1) that
 *     is, else 0; g_y likewise; both 0 when z is +inf.
 *   Pass i = 0 .. levels-1, s = 2^i, per valid pixel p.  Y = (0.2126f*I_r + 0.7152f*I_g) + 0.0722f*I_b of the current image.
 *     Vg_p = (sum of k3 * V_q) / (sum of k3) over the 3x3 adjacent pixels q that are in the image and valid, rows bottom to top, x
 *     ascending, k3 = (1 2 1; 2 4 2; 1 2 1), both sums from 0.
 *     Taps q = p + s*(dx, dy), dy = -2..2 outer, dx = -2..2 inner, ascending; taps outside the image or invalid are skipped.
 *     h = k[|dx|] * k[|dy|], k = (3/8, 1/4, 1/16).  The centre tap has w = h.  For the others:
 *       w_n: normal off: 1.  Both without normal: 1; one without: 0; else fmaxf(0, (n^p_x*n^q_x + n^p_y*n^q_y) + n^p_z*n^q_z), squared
 *         normal_squarings times.
 *       x_z: depth off: 0.  Both depths +inf: 0; one: the tap is skipped; else fabsf(z_p - z_q) / (sigma_z * (fabsf(g_x*(float)(s*dx) +
 *         g_y*(float)(s*dy)) + 0.001f*z_p)).
 *       x_l: stderr3 off: 0; else fabsf(Y_p - Y_q) / (sigma_l * sqrtf(Vg_p) + 1e-6f).
 *       w = ((h * w_n) * E(x_z)) * E(x_l).
 *     In tap order from 0: W += w, J_c += w * I_q,c, U += (w*w) * V_q.  Then I'_p,c = J_c / W, V'_p = U / (W*W)  (W >= 9/64).
 *   Finish.  out_c = I_c * a_c.
 * Scratch (two ping-pong images and the packed guides, 56 bytes per pixel) belongs to the scene handle, is allocated on first use and
 * regrown when a larger image comes.  "At most one render in flight per vk_scene" covers these calls; they touch nothing that describes
 * vk_render's last frame and no vk_progress handle.
 * VK_ERR_BAD_ARG, nothing enqueued, out untouched: null scene / dp / color / out, zero or too large a size (vk_render's limits),
 * levels outside 1..8, normal_squarings > 10, a sigma_l, sigma_z or albedo_floor that is not finite or not > 0, flags != 0, out
 * overlapping an input.                                                                                                           */
typedef struct vk_denoise_params {
    uint32_t width, height;
    uint32_t levels;            /* 1..8 passes; pass i has tap spacing s = 2^i            */
    uint32_t normal_squarings;  /* 0..10: w_n = max(0, cos)^(2^normal_squarings)          */
    float sigma_l;              /* colour tolerance, in standard errors of the luminance  */
    float sigma_z;              /* depth tolerance, in units of the local depth slope     */
    float albedo_floor;         /* > 0: demodulation divides by max(albedo, albedo_floor) */
    uint32_t flags;             /* 0                                                       */
} vk_denoise_params;
/* levels 5, normal_squarings 7, sigma_l 4, sigma_z 1, albedo_floor 1e-3 (what was tried).  Touches no device. */
int vk_denoise_default_params(uint32_t width, uint32_t height, vk_denoise_params *out);
/* host buffers; blocking.  stats_out: samples = pixels, kernel_ms (HIP events around the passes), kernel_launches = 1 + levels */
int vk_denoise(vk_scene *scene, const vk_denoise_params *dp, const float *color, const float *stderr3,
               const float *albedo, const float *normal, const float *depth, float *out, vk_stats *stats_out);
/* device buffers on the scene's device (devices[0] of a multi-device scene), enqueued on hip_stream, no host wait */
int vk_denoise_device(vk_scene *scene, const vk_denoise_params *dp, const void *d_color, const void *d_stderr3,
                      const void *d_albedo, const void *d_normal, const void *d_depth, void *d_out, void *hip_stream);
/* vk_progress_stderr into device memory on the scene's device: the same formula in double with the same operation order, bit-identical
 * to the host call; the same argument checks; this partition's pixels only, others untouched.  Waits for the handle's last step, then
 * enqueues on hip_stream without a further host wait.  A handle on a multi-device scene returns VK_ERR_UNSUPPORTED (its moments live on
 * several devices): vk_progress_stderr stays the way there. */
int vk_progress_stderr_device(vk_progress *pr, void *d_out, void *hip_stream);

/* ---- temporal accumulation: reproject and blend the frames of a moving camera (additive symbols of ABI 7) -----------------------------
 * replaces: nothing (the reference's frame loop, main.rs:176, starts every frame from nothing).  The temporal half of SVGF, in front of
 * vk_denoise: a frame's noisy colour, its standard error, its first-hit buffers and its camera go in; each pixel's first hit is
 * reprojected into the previous frame's camera, the accumulated history is fetched there with validated bilinear taps and blended with
 * the frame, the variance is propagated, and the result is kept as the next frame's history.  out_color and out_stderr3 have the shapes
 * vk_denoise takes: render -> AOV -> accumulate -> denoise.  All images are in vk_render's f32 layout (y = 0 the bottom row): color,
 * stderr3, albedo, normal, out_color and out_stderr3 3 floats per pixel, depth and out_history 1.  color, normal, depth, out_color and cam
 * are required (no reprojection without geometry); albedo may be NULL (no demodulation); stderr3 may be NULL (the variance is 0;
 * out_stderr3 must be NULL too); out_stderr3 and out_history may be NULL.  The call works on the whole image (no tile partition), on the
 * scene's device (devices[0] of a multi-device scene).  The scene is static by construction (a description is immutable after
 * vk_scene_create); the caller changes the seed per frame, so that frames are independent.
 *
 * The definition, exactly.  Everything is f32, unfused, in the order written, with + - * /, sqrtf, fabsf, fmaxf, fminf, floorf and
 * compares only; a . b = (a_x*b_x + a_y*b_y) + a_z*b_z; tests/temporal_ref.py restates it in numpy and the two agree bit for bit.
 * Primes denote the previous frame: its camera (o' = origin, llc', H' = horizontal, V' = vertical, w') and its stored history.
 *   Prepare, per pixel p = (x, y).  a_c = fmaxf(albedo_c, albedo_floor), or 1 without albedo; I_c = color_c / a_c; S_c = stderr_c / a_c,
 *     Vc_c = S_c * S_c (0 without stderr3): the variance per component, so that the output feeds vk_denoise's stderr3.  p is INVALID if a
 *     component of color (or of stderr3, when given) is not finite: out_color is its color and out_stderr3 its stderr3, unchanged,
 *     out_history 0; it is stored with N = 0 and is never a tap.  Normal: l2 = n . n; l2 < 1e-12f or not finite: p has NO NORMAL; else
 *     n^ = n / sqrtf(l2).  Depth: z = depth if finite, else +inf (a miss).
 *   First-hit point.  s = ((float)x + 0.5f) / (float)(width-1), t = ((float)y + 0.5f) / (float)(height-1) (main.rs:187); d = ((llc + H*s)
 *     + V*t) - origin: the pixel centre through the lens centre (the lens offset is ignored); len = sqrtf(d . d).  A hit: e = (origin +
 *     d * (z / len)) - o'.  A miss: e = d (a point at infinity: only the rotation matters).
 *   Projection into the previous camera.  q = llc' - o', fw = -(q . w'), ew = -(e . w').  Not ew > 0: no history.  g = e * (fw / ew) - q;
 *     s' = (g . H') / (H' . H'), t' = (g . V') / (V' . V'); px = s' * (float)(width-1) - 0.5f, py = t' * (float)(height-1) - 0.5f.  Not
 *     (px > -1 and px < (float)width and py > -1 and py < (float)height): no history.
 *   Taps.  x0 = floorf(px), fx = px - x0, y0 = floorf(py), fy = py - y0.  Four taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), in
 *     that order, with the weights b = (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy.  A tap outside the image is skipped.  A tap q is
 *     CONSISTENT when N'_q > 0, and: depth — for a miss pixel z'_q is +inf; for a hit, with ze = sqrtf(e . e), fabsf(z'_q - ze) <=
 *     depth_tol * ze; and normal — both without a normal: consistent; one without: not; else n^_p . n^'_q >= normal_cos_min.
 *   Sums over the consistent taps, in tap order, each from 0: W += b, J_c += b * I'_q,c, U_c += b * V'_q,c, M += b * N'_q.
 *   Blend.  If W >= 0.01f: I_h = J / W, V_h = U / W, N_h = M / W (the variance of resampled, correlated taps is bounded by their weighted
 *     mean: an upper bound, on purpose); N = fminf(N_h + 1.0f, (float)max_history), alpha = 1.0f / N, k = 1.0f - alpha; I'_c = k * I_h,c
 *     + alpha * I_c, V'_c = (k*k) * V_h,c + (alpha*alpha) * Vc_c.  Otherwise (also: the first frame after create or reset): no history,
 *     I' = I, V' = Vc, N = 1.
 *   Finish.  out_color_c = I'_c * a_c, out_stderr3_c = sqrtf(V'_c) * a_c, out_history = N.  (I', V', N, n^, z) and cam become the history.
 *     vk_temporal_info.pixels_with_history counts the pixels of the last frame that took the W >= 0.01f branch.
 * What this is not.  First-hit reprojection is wrong for what is seen in a mirror or through glass: such pixels keep their history and
 * lag; only max_history bounds the lag.  Nothing detects a changed scene (impossible through this ABI).  Depth of field and motion blur
 * are reprojected through the lens centre at the averaged depth.
 * The handle owns the history on the scene's device: two ping-pong sets of three float4 planes, (I_r, I_g, I_b, N), (V_r, V_g, V_b, z),
 * (n^_x, n^_y, n^_z, -), 48 bytes per pixel each, and the previous camera.  "At most one render in flight per vk_scene" covers these
 * calls too; they touch nothing that describes vk_render's last frame and no vk_progress handle.
 * VK_ERR_BAD_ARG, nothing enqueued, handle and outputs untouched: null required pointers, width or height < 2 or beyond vk_render's
 * limits, max_history outside 1..65535, depth_tol not finite or not > 0, normal_cos_min not finite or outside -1..1, albedo_floor not
 * finite or not > 0, flags != 0, an output overlapping an input or another output, out_stderr3 without stderr3.  Any other error
 * (VK_ERR_HIP, VK_ERR_OOM) may come after the frame was enqueued: the handle may have advanced to it while the host outputs were not
 * written; vk_temporal_reset before the handle is used again.                                                                       */
typedef struct vk_temporal vk_temporal;            /* opaque; owns the history, on the scene's device */
typedef struct vk_temporal_params {
    uint32_t width, height;      /* >= 2 each (the pixel-centre mapping divides by width-1), vk_render's upper limits */
    uint32_t max_history;        /* 1..65535: the history length N is capped here; blend factor alpha = 1/N */
    float depth_tol;             /* a tap is consistent when |z_tap - z_expected| <= depth_tol * z_expected   (finite, > 0) */
    float normal_cos_min;        /* ... and n_p . n_tap >= normal_cos_min                                     (finite, -1..1) */
    float albedo_floor;          /* > 0, as vk_denoise_params.albedo_floor */
    uint32_t flags;              /* 0 */
} vk_temporal_params;
typedef struct vk_temporal_info { uint32_t frames; uint32_t width, height; uint64_t pixels_with_history; /* of the last frame */ } vk_temporal_info;
/* max_history 32, depth_tol 0.02, normal_cos_min 0.9, albedo_floor 1e-3 (the sweep).  Touches no device. */
int vk_temporal_default_params(uint32_t width, uint32_t height, vk_temporal_params *out);
int vk_temporal_create(vk_scene *scene, const vk_temporal_params *tp, vk_temporal **out);
/* host buffers; blocking.  stats_out: samples = pixels, kernel_ms (HIP events around the kernel), kernel_launches = 1 */
int vk_temporal_accumulate(vk_temporal *t, const vk_camera *cam, const float *color, const float *stderr3, const float *albedo,
                           const float *normal, const float *depth, float *out_color, float *out_stderr3, float *out_history, vk_stats *stats_out);
/* device buffers on the scene's device, enqueued on hip_stream, no host wait; successive frames of one handle go on one stream */
int vk_temporal_accumulate_device(vk_temporal *t, const vk_camera *cam, const void *d_color, const void *d_stderr3, const void *d_albedo,
                                  const void *d_normal, const void *d_depth, void *d_out_color, void *d_out_stderr3, void *d_out_history, void *hip_stream);
int vk_temporal_reset(vk_temporal *t);            /* forget the history; the next frame is a first frame */
int vk_temporal_get_info(vk_temporal *t, vk_temporal_info *out);   /* waits for the last frame */
void vk_temporal_destroy(vk_temporal *t);          /* NULL: nothing; destroy before its scene */

/* ---- ID mattes: per-pixel object and material coverage of primary rays (additive symbols of ABI 7) ---------------------------------
 * replaces: nothing.  Next to vk_render_aov's and vk_render_guides' buffers, the third thing a compositor takes: WHICH object, or which
 * material, each pixel shows, and with how much of its area (an "ID matte" or Cryptomatte AOV: per-object masks, selection outlines,
 * picking, per-object statistics).  Everything here is an integer: every result is exact and no sample is ever dropped.
 *   Samples.  first_sample .. first_sample + spp - 1, spp = params->samples_per_pixel.  Sample s of pixel (x, y) is exactly
 *     vk_render_aov's: the stream (seed, y * width + x, s), the camera's draws first, the walk with tmin 0.001 and tmax inf on the tree
 *     view vk_render_aov walks (the tree as handed over; the rebuilt tree under VK_SCENE_FAST_ACCEL), a ConstantMedium's draws
 *     continuing that stream.
 *   The id of a sample.  VK_MATTE_OBJECT: vk_hit.object as vk_trace_rays names it — VK_MAKE_REF(kind, index) of the description record
 *     whose own hit() produced the winner, without the flip bit; a Boxy reports its face's Rect, a medium its VK_KIND_MEDIUM record.
 *     VK_MATTE_MATERIAL: the hit record's material index; for a medium its phase function's material.  A miss is VK_MATTE_BACKGROUND
 *     under either kind: an id like any other, which takes a slot.
 *   The table of a pixel, exact and in a fixed order: `ranks` slots (1..8), empty at first.  Samples are taken in increasing order.  A
 *     sample whose id is in a slot adds 1 to that slot; otherwise, if a slot is free, it takes it with count 1; otherwise it adds 1 to
 *     the pixel's overflow (first come, no eviction).  At the end the used slots are sorted by count descending, ties by id ascending;
 *     an unused slot is written as (id 0, count 0).  ids[pix * ranks + r], counts[pix * ranks + r], overflow[pix], pix = y * width + x,
 *     y = 0 the bottom row.  overflow may be NULL; ids and counts may not.  Pixels outside the call's tile partition are left
 *     untouched.  One value per (scene, camera, seed, window, kind, ranks), whatever the launch shape; in every pixel
 *     sum(counts) + overflow == spp.
 *   vk_matte_merge (host code, no device) folds table b into table a, pixel by pixel: b's used slots in b's order, the same rule for
 *     each (found: add its count; a free slot: take it; else overflow += count), then overflow += overflow_b, and the slots are sorted
 *     again.  The three overflow pointers of a call are all given or all NULL.  A frame's windows merged in any order equal the one
 *     call over their union wherever that call's overflow is 0, and the merged overflow is 0 exactly there.
 *   vk_matte_mask (host code): mask_out[pix] = (float)(sum of the counts of the slots whose id is in want[0 .. n_want)) /
 *     (float)n_samples.  A set of ids, because one box is six face ids.
 *   Arguments: vk_render's checks, in the same words; output_format, max_depth, integrator and the background are not read.
 *     VK_ERR_BAD_ARG with nothing enqueued and every output untouched for a null mp, ids or counts, an unknown kind, ranks outside 1..8,
 *     flags != 0, first_sample + spp > 2^32 - 1.  vk_matte_merge and vk_matte_mask refuse null arrays with n_pixels > 0, ranks outside
 *     1..8, n_samples == 0, a null want with n_want > 0.
 *   Scene state: vk_render_aov's rules.  The call is the scene's one render in flight and runs on devices[0] of a multi-device scene;
 *     it touches nothing of vk_render's last frame, nor the launch log, any vk_progress or vk_temporal handle, or vk_render_aov's own
 *     results and times.  It uploads the tables that map device primitives back to the description on first use, as the first ray
 *     query does.  stats_out: samples = partition pixels x spp, kernel_ms, kernel_launches.
 *   What this is not.  Ids are not followed through mirrors and glass: a glass sphere is its own id, whatever is seen in it
 *     (vk_render_guides does not keep the name of the hit it reports).                                                             */
enum { VK_MATTE_OBJECT = 0, VK_MATTE_MATERIAL = 1 };
#define VK_MATTE_BACKGROUND 0xFFFFFFFFu
#define VK_MATTE_MAX_RANKS 8u
typedef struct vk_matte_params { uint32_t kind, ranks, flags, _pad; } vk_matte_params;   /* 16 bytes */
/* VK_MATTE_OBJECT, 6 ranks, flags 0; touches no device */
int vk_matte_default_params(vk_matte_params *out);
int vk_render_mattes(vk_scene *scene, const vk_camera *cam, const vk_render_params *params, uint32_t first_sample,
                     const vk_matte_params *mp, uint32_t *ids, uint32_t *counts, uint32_t *overflow, vk_stats *stats_out);
int vk_matte_merge(uint32_t ranks, uint64_t n_pixels, uint32_t *ids, uint32_t *counts, uint32_t *overflow,
                   const uint32_t *ids_b, const uint32_t *counts_b, const uint32_t *overflow_b);
int vk_matte_mask(uint32_t ranks, uint64_t n_pixels, const uint32_t *ids, const uint32_t *counts, uint32_t n_samples,
                  const uint32_t *want, uint32_t n_want, float *mask_out);

/* test/diagnostic entry points (vk_debug_*) are declared in vecchio_amd_debug.h */

#ifdef __cplusplus
}
#endif
#endif /* VECCHIO_AMD_H */
