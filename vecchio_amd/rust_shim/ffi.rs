// ffi.rs — Rust-side binding of include/vecchio_amd.h for browserdotsys/vecchio.
//
// UNCOMPILED SOURCE: there is no Rust toolchain in the build image (no cargo/rustc), so this
// file has never been through rustc.  It is the binding a vecchio maintainer would add as
// `src/ffi.rs` (+ `mod ffi;` in main.rs) together with the `flatten()` methods sketched in
// flatten.rs; INTEGRATION.md walks through the three edits.  The C++ twin of this code that IS
// compiled and tested lives in vecchio_amd/host/ (same structure, same record layout).
#![allow(non_camel_case_types, dead_code)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

pub type vk_ref = u32;
pub const VK_ABI_VERSION: u32 = 7;
pub const VK_PROBE_COEFFS: u32 = 9;
pub const VK_SCENE_FAST_ACCEL: u32 = 1;
pub const VK_SCENE_REFERENCE_TREE: u32 = 2;
pub const VK_SCENE_EMPIRICAL_TREES: u32 = 4;
pub const VK_SCENE_RCCL_GATHER: u32 = 8;
pub const VK_PROGRESS_STDERR: u32 = 1;
pub const VK_REF_FLIP: u32 = 0x0800_0000;
pub const VK_KIND_BVH: u32 = 1;
pub const VK_KIND_SPHERE: u32 = 2;
pub const VK_KIND_MOVING_SPHERE: u32 = 3;
pub const VK_KIND_RECT: u32 = 4;
pub const VK_KIND_LIST: u32 = 5;
pub const VK_KIND_MEDIUM: u32 = 6;
pub const VK_KIND_TRANSLATE: u32 = 7;
pub const VK_KIND_ROTATE: u32 = 8;
pub fn make_ref(kind: u32, index: usize) -> vk_ref { (kind << 28) | (index as u32 & 0x07FF_FFFF) }

#[repr(C)] #[derive(Copy, Clone)] pub struct vk_bvh_node { pub bb_min: [f32; 3], pub bb_max: [f32; 3], pub left: vk_ref, pub right: vk_ref }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_sphere { pub center: [f32; 3], pub radius: f32, pub material: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_moving_sphere { pub center0: [f32; 3], pub center1: [f32; 3], pub time0: f32, pub time1: f32, pub radius: f32, pub material: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_rect { pub c0: f32, pub c1: f32, pub d0: f32, pub d1: f32, pub k: f32, pub axis0: u8, pub axis1: u8, pub axis2: u8, pub _pad: u8, pub material: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_list { pub first: u32, pub count: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_medium { pub boundary: vk_ref, pub neg_inv_density: f32, pub material: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_translate { pub child: vk_ref, pub offset: [f32; 3] }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_rotate { pub child: vk_ref, pub axis: u32, pub sin_theta: f32, pub cos_theta: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_material { pub kind: u32, pub texture: u32, pub param: f32, pub a: u32, pub b: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_texture { pub kind: u32, pub color: [f32; 3], pub a: u32, pub b: u32, pub scale: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_image { pub width: u32, pub height: u32, pub rgb: *const u8 }
#[repr(C)] #[derive(Copy, Clone)] pub struct vk_perlin { pub ranvec: [[f32; 3]; 256], pub perm_x: [u32; 256], pub perm_y: [u32; 256], pub perm_z: [u32; 256] }

#[repr(C)]
pub struct vk_scene_desc {
    pub abi_version: u32,
    pub n_bvh: u32, pub bvh: *const vk_bvh_node,
    pub n_spheres: u32, pub spheres: *const vk_sphere,
    pub n_moving_spheres: u32, pub moving_spheres: *const vk_moving_sphere,
    pub n_rects: u32, pub rects: *const vk_rect,
    pub n_lists: u32, pub lists: *const vk_list,
    pub n_list_items: u32, pub list_items: *const vk_ref,
    pub n_media: u32, pub media: *const vk_medium,
    pub n_translates: u32, pub translates: *const vk_translate,
    pub n_rotates: u32, pub rotates: *const vk_rotate,
    pub n_materials: u32, pub materials: *const vk_material,
    pub n_textures: u32, pub textures: *const vk_texture,
    pub n_images: u32, pub images: *const vk_image,
    pub n_perlins: u32, pub perlins: *const vk_perlin,
    pub world: vk_ref,
    pub n_lights: u32, pub lights: *const vk_ref,
    pub flags: u32,             // 0 = the handed-over tree's results (exact re-treeing of sphere-only worlds, see vecchio_amd.h); VK_SCENE_*
}

#[repr(C)] #[derive(Copy, Clone)]
pub struct vk_camera {          // the ten fields of main.rs:57-68 (add #[repr(C)] there, or copy)
    pub origin: [f32; 3], pub lower_left_corner: [f32; 3], pub horizontal: [f32; 3], pub vertical: [f32; 3],
    pub u: [f32; 3], pub v: [f32; 3], pub w: [f32; 3], pub lens_radius: f32, pub time0: f32, pub time1: f32,
}

#[repr(C)] #[derive(Copy, Clone)]
pub struct vk_render_params {
    pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub max_depth: u32, pub seed: u64,
    pub integrator: u32, pub background: u32, pub background_color: [f32; 3], pub tile_rank: u32, pub tile_world: u32,
    pub output_format: u32,     // VK_OUTPUT_F32 = 0 | VK_OUTPUT_RGB8 = 1 (Vec3::to_color + top-down rows fused, vec3.rs:54-61, main.rs:209)
}

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_stats { pub samples: u64, pub seconds: f64, pub kernel_ms: f64, pub kernel_launches: u32, pub scene_in_lds: u32, pub clamped_samples: u64 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_progress_info { pub samples_done: u32, pub samples_budget: u32, pub steps: u32, pub flags: u32, pub clamped_samples: u64 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_adaptive_params { pub abs_tol: f32, pub rel_tol: f32, pub min_samples: u32, pub min_steps: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_adaptive_info { pub tiles_total: u32, pub tiles_active: u32, pub samples_rendered: u64 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_denoise_params { pub width: u32, pub height: u32, pub levels: u32, pub normal_squarings: u32, pub sigma_l: f32, pub sigma_z: f32, pub albedo_floor: f32, pub flags: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_guide_params { pub max_bounces: u32, pub fuzz_max: f32, pub flags: u32 }

// ray queries: a caller-supplied ray (tmax: f32::INFINITY for main.rs:130's call), its closest hit, the batch parameters
pub const VK_RAY_TMIN: f32 = 0.001;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_ray { pub origin: [f32; 3], pub tmax: f32, pub direction: [f32; 3], pub time: f32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_hit { pub p: [f32; 3], pub t: f32, pub normal: [f32; 3], pub u: f32, pub v: f32, pub hit: u32, pub front: u32, pub material: u32, pub object: vk_ref, pub medium: u32, pub _pad: [u32; 2] }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_trace_params { pub seed: u64, pub first_index: u64, pub flags: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_radiance_params { pub seed: u64, pub first_index: u64, pub samples_per_ray: u32, pub first_sample: u32, pub max_depth: u32, pub integrator: u32, pub background: u32, pub background_color: [f32; 3], pub flags: u32, pub _pad: u32 }

// shade queries: the state of a path between bounces, one bounce's result, the call's parameters
pub const VK_SHADE_MISS: u32 = 0;
pub const VK_SHADE_SCATTERED: u32 = 1;
pub const VK_SHADE_ENDED: u32 = 2;
pub const VK_SHADE_BAD_HIT: u32 = 3;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_path_state { pub thr: [f32; 3], pub depth: u32, pub acc: [f32; 3], pub counter: u32, pub seed: u64, pub pixel: u32, pub sample: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_shaded { pub next: vk_ray, pub state: vk_path_state, pub status: u32, pub lobe: u32, pub _pad: [u32; 2] }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_shade_params { pub max_depth: u32, pub integrator: u32, pub background: u32, pub background_color: [f32; 3], pub flags: u32, pub _pad: u32 }

// path batches: what a handle holds, and what one vk_paths_step did
pub const VK_PATHS_LIVE: u32 = 1;
pub const VK_PATHS_CULLED: u32 = 4;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_paths_info { pub capacity: u64, pub started: u64, pub live: u64, pub retired: [u64; 5], pub bounces: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_paths_step_info { pub traced: u64, pub live: u64, pub missed: u64, pub ended: u64, pub bad: u64, pub bounces: u32, pub kernel_launches: u32, pub kernel_ms: f64, pub seconds: f64 }

// the termination rule of a path batch handle (vk_roulette_set)
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_roulette_params { pub first_depth: u32, pub q_min: f32, pub q_max: f32, pub flags: u32 }

// films: a window of camera paths to emit, and a film's counters
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_film_window { pub x0: u32, pub y0: u32, pub width: u32, pub height: u32, pub first_sample: u32, pub n_samples: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_film_info { pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub _pad: u32, pub emitted: u64, pub deposited: u64, pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64 }

// a film's error moments and tile map: what one vk_adapt_close left
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_adapt_info { pub samples_done: u32, pub steps: u32, pub tiles_total: u32, pub tiles_active: u32, pub pixels_active: u64, pub samples_rendered: u64 }

// reconstruction filters: an accumulator's filter, and its counters
pub const VK_SPLAT_BOX: u32 = 0;
pub const VK_SPLAT_TENT: u32 = 1;
pub const VK_SPLAT_MITCHELL: u32 = 2;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_splat_params { pub filter: u32, pub radius: f32, pub b: f32, pub c: f32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_splat_info { pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub filter: u32, pub deposited: u64, pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64, pub contributions: u64 }

// ID mattes: the kind of id and the table's size
pub const VK_MATTE_OBJECT: u32 = 0;
pub const VK_MATTE_MATERIAL: u32 = 1;
pub const VK_MATTE_BACKGROUND: u32 = 0xFFFF_FFFF;
pub const VK_MATTE_MAX_RANKS: u32 = 8;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_matte_params { pub kind: u32, pub ranks: u32, pub flags: u32, pub _pad: u32 }

// robust film: an accumulator's buckets and estimator, and its counters
pub const VK_ROBUST_MEAN: u32 = 0;
pub const VK_ROBUST_TRIM: u32 = 1;
pub const VK_ROBUST_GINI: u32 = 2;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_robust_params { pub buckets: u32, pub mode: u32, pub trim: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_robust_info { pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub buckets: u32, pub deposited: u64, pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64, pub _reserved: u64 }

// light-path layers: a rule, the rule set of a tracker, and its counters
pub const VK_LPE_SKY: u32 = 1;
pub const VK_LPE_EMIT: u32 = 5;
pub const VK_LPE_OTHER: u32 = 14;
pub const VK_LPE_BAD: u32 = 15;
pub const VK_LPE_ALL: u32 = 0xFFFF_FFFF;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_lpe_rule { pub sig_mask: u32, pub sig_value: u32, pub status_mask: u32, pub depth_min: u32, pub depth_max: u32, pub emitter: u32, pub layer: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone)]
pub struct vk_lpe_params { pub n_layers: u32, pub rest_layer: u32, pub n_rules: u32, pub _pad: u32, pub rules: *const vk_lpe_rule }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_lpe_info { pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub n_layers: u32, pub rest_layer: u32, pub n_rules: u32, pub capacity: u64, pub deposited: u64, pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64, pub recorded: u64 }

// display transform: the meter's and the encode's parameters, what a meter found, a handle's counts
pub const VK_TONE_CLAMP: u32 = 0;
pub const VK_TONE_REINHARD: u32 = 1;
pub const VK_TONE_HABLE: u32 = 2;
pub const VK_TONE_ACES: u32 = 3;
pub const VK_TONE_TRANSFER_REFERENCE: u32 = 0;
pub const VK_TONE_TRANSFER_SRGB: u32 = 1;
pub const VK_TONE_TRANSFER_GAMMA22: u32 = 2;
pub const VK_TONE_USE_METERED: u32 = 1;
pub const VK_TONE_DITHER: u32 = 2;
pub const VK_TONE_METER_EMPTY: u32 = 1;
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_tone_meter_params { pub key: f32, pub low_fraction: f32, pub high_fraction: f32, pub blend: f32, pub min_log2: f32, pub max_log2: f32, pub _pad: [u32; 2] }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_tone_meter_info { pub log2_target: f64, pub log2_used: f64, pub binned: u64, pub below: u64, pub above: u64, pub nonfinite: u64, pub exposure: f32, pub flags: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_tone_params { pub curve: u32, pub transfer: u32, pub flags: u32, pub _pad: u32, pub exposure: f32, pub white: f32, pub seed: u64 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_tone_info { pub width: u32, pub height: u32, pub loads: u64, pub meters: u64, pub encodes: u64, pub exposure: f32, pub metered: u32, pub log2_used: f64 }

// non-local means: the filter's parameters, and what a handle holds and last did
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_nlm_params { pub search_radius: u32, pub patch_radius: u32, pub k: f32, pub alpha: f32, pub albedo_floor: f32, pub flags: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_nlm_info { pub width: u32, pub height: u32, pub loaded: u32, pub has_albedo: u32, pub loads: u64, pub filters: u64, pub last_launches: u32, pub last_form: u32, pub last_kernel_ms: f64, pub scratch_bytes: u64 }

// glare: the stage's parameters, and what a handle holds and last did
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_glare_params { pub levels: u32, pub strength: f32, pub falloff: f32, pub threshold: f32, pub flags: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_glare_info { pub width: u32, pub height: u32, pub applies: u64, pub last_levels: u32, pub last_form: u32, pub last_launches: u32, pub _pad: u32, pub last_kernel_ms: f64, pub scratch_bytes: u64 }

// point-spread function: the stage's parameters, and what a handle holds and last did
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_psf_params { pub strength: f32, pub threshold: f32, pub form: u32, pub flags: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_psf_info { pub width: u32, pub height: u32, pub K: u32, pub Px: u32, pub Py: u32, pub kmax: u32, pub last_form: u32, pub last_launches: u32, pub loads: u64, pub applies: u64, pub last_kernel_ms: f64, pub scratch_bytes: u64 }

// guided upsampling: the filter's parameters, and what a handle holds and last did
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_upsample_params { pub sigma_z: f32, pub normal_squarings: u32, pub albedo_floor: f32, pub flags: u32, pub _pad: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_upsample_info { pub width_lo: u32, pub height_lo: u32, pub width_hi: u32, pub height_hi: u32, pub loaded: u32, pub guides: u32, pub loads: u64, pub applies: u64, pub last_form: u32, pub last_launches: u32, pub last_kernel_ms: f64, pub scratch_bytes: u64, pub fallback_pixels: u64, pub empty_pixels: u64 }

// regeneration: what one vk_regen_step did
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_regen_info { pub traced: u64, pub live: u64, pub remaining: u64, pub emitted: u64, pub missed: u64, pub ended: u64, pub bad: u64, pub bounces: u32, pub kernel_launches: u32, pub kernel_ms: f64, pub seconds: f64 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_temporal_params { pub width: u32, pub height: u32, pub max_history: u32, pub depth_tol: f32, pub normal_cos_min: f32, pub albedo_floor: f32, pub flags: u32 }

#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct vk_temporal_info { pub frames: u32, pub width: u32, pub height: u32, pub pixels_with_history: u64 }

#[repr(C)] pub struct vk_scene { _private: [u8; 0] }
#[repr(C)] pub struct vk_progress { _private: [u8; 0] }
#[repr(C)] pub struct vk_temporal { _private: [u8; 0] }
#[repr(C)] pub struct vk_paths { _private: [u8; 0] }
#[repr(C)] pub struct vk_film { _private: [u8; 0] }
#[repr(C)] pub struct vk_splat { _private: [u8; 0] }
#[repr(C)] pub struct vk_robust { _private: [u8; 0] }
#[repr(C)] pub struct vk_lpe { _private: [u8; 0] }
#[repr(C)] pub struct vk_tone { _private: [u8; 0] }
#[repr(C)] pub struct vk_nlm { _private: [u8; 0] }
#[repr(C)] pub struct vk_glare { _private: [u8; 0] }
#[repr(C)] pub struct vk_upsample { _private: [u8; 0] }
#[repr(C)] pub struct vk_psf { _private: [u8; 0] }

#[link(name = "vecchio_amd")]
extern "C" {
    pub fn vk_abi_version() -> c_int;
    pub fn vk_device_count() -> c_int;
    pub fn vk_last_error() -> *const c_char;
    pub fn vk_scene_create(desc: *const vk_scene_desc, device: c_int, out: *mut *mut vk_scene) -> c_int;
    pub fn vk_scene_create_multi(desc: *const vk_scene_desc, devices: *const c_int, n_devices: c_int, out: *mut *mut vk_scene) -> c_int;
    pub fn vk_scene_destroy(scene: *mut vk_scene);
    pub fn vk_render(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, rgb_out: *mut f32, stats: *mut vk_stats) -> c_int;
    pub fn vk_render_device(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, d_rgb: *mut c_void, stream: *mut c_void, stats: *mut vk_stats) -> c_int;
    pub fn vk_scene_last_kernel_ms(scene: *mut vk_scene, ms_out: *mut f64) -> c_int;
    pub fn vk_scene_last_clamped_samples(scene: *mut vk_scene, count_out: *mut u64) -> c_int;
    pub fn vk_scene_last_requeued_samples(scene: *mut vk_scene, count_out: *mut u64) -> c_int;
    pub fn vk_tile_slab_bytes(width: u32, height: u32, output_format: u32, tile_rank: u32, tile_world: u32) -> usize;
    pub fn vk_pack_tiles_device(scene: *mut vk_scene, d_fb: *const c_void, width: u32, height: u32, output_format: u32, tile_rank: u32, tile_world: u32, d_slab: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn vk_unpack_tiles_device(scene: *mut vk_scene, d_slab: *const c_void, width: u32, height: u32, output_format: u32, tile_rank: u32, tile_world: u32, d_img: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn vk_progress_create(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, flags: u32, out: *mut *mut vk_progress) -> c_int;
    pub fn vk_progress_step(pr: *mut vk_progress, n_samples: u32, out: *mut c_void, stats: *mut vk_stats) -> c_int;
    pub fn vk_progress_step_device(pr: *mut vk_progress, n_samples: u32, d_out: *mut c_void, stream: *mut c_void, stats: *mut vk_stats) -> c_int;
    pub fn vk_progress_reset(pr: *mut vk_progress, cam: *const vk_camera) -> c_int;
    pub fn vk_progress_stderr(pr: *mut vk_progress, out: *mut f32) -> c_int;
    pub fn vk_progress_get_info(pr: *mut vk_progress, out: *mut vk_progress_info) -> c_int;
    pub fn vk_progress_destroy(pr: *mut vk_progress);
    pub fn vk_progress_set_adaptive(pr: *mut vk_progress, ap: *const vk_adaptive_params) -> c_int;
    pub fn vk_progress_tile_samples(pr: *mut vk_progress, out: *mut u32, info: *mut vk_adaptive_info) -> c_int;
    // first-hit buffers (additive symbols of ABI 7): any of the four may be null, not all four
    pub fn vk_render_aov(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, first_sample: u32,
                         albedo: *mut f32, normal: *mut f32, depth: *mut f32, coverage: *mut f32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_render_aov_device(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, first_sample: u32,
                                d_albedo: *mut c_void, d_normal: *mut c_void, d_depth: *mut c_void, d_coverage: *mut c_void,
                                hip_stream: *mut c_void, stats_out: *mut vk_stats) -> c_int;
    // specular guides (additive symbols of ABI 7): the first-hit buffers followed through mirrors and glass; any of the five may be null
    pub fn vk_guide_default_params(out: *mut vk_guide_params) -> c_int;
    pub fn vk_render_guides(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, first_sample: u32,
                            gp: *const vk_guide_params, albedo: *mut f32, normal: *mut f32, depth: *mut f32, coverage: *mut f32,
                            bounces: *mut f32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_render_guides_device(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, first_sample: u32,
                                   gp: *const vk_guide_params, d_albedo: *mut c_void, d_normal: *mut c_void, d_depth: *mut c_void,
                                   d_coverage: *mut c_void, d_bounces: *mut c_void, hip_stream: *mut c_void,
                                   stats_out: *mut vk_stats) -> c_int;
    // ray queries (additive symbols of ABI 7): world.hit(&ray, 0.001, tmax) for rays the caller supplies; hits[i] answers rays[i]
    pub fn vk_trace_rays(scene: *mut vk_scene, params: *const vk_trace_params, rays: *const vk_ray, n_rays: u64, hits: *mut vk_hit,
                         stats_out: *mut vk_stats) -> c_int;
    pub fn vk_trace_rays_device(scene: *mut vk_scene, params: *const vk_trace_params, d_rays: *const c_void, n_rays: u64,
                                d_hits: *mut c_void, hip_stream: *mut c_void, stats_out: *mut vk_stats) -> c_int;
    // occlusion queries (additive symbols of ABI 7): occluded[i] = hits[i].hit of vk_trace_rays on the same arguments, one byte per ray
    pub fn vk_trace_occluded(scene: *mut vk_scene, params: *const vk_trace_params, rays: *const vk_ray, n_rays: u64, occluded: *mut u8,
                             stats_out: *mut vk_stats) -> c_int;
    pub fn vk_trace_occluded_device(scene: *mut vk_scene, params: *const vk_trace_params, d_rays: *const c_void, n_rays: u64,
                                    d_occluded: *mut c_void, hip_stream: *mut c_void, stats_out: *mut vk_stats) -> c_int;
    // radiance queries (additive symbols of ABI 7): rgb_out[i] = the mean of samples_per_ray samples of ray_color(rays[i]), 3 floats per ray
    pub fn vk_trace_radiance(scene: *mut vk_scene, params: *const vk_radiance_params, rays: *const vk_ray, n_rays: u64, rgb_out: *mut f32,
                             stats_out: *mut vk_stats) -> c_int;
    // irradiance queries (additive symbols of ABI 7): a point is a vk_ray whose origin is the position and whose direction is the surface
    // normal; rgb_out[i] = the mean radiance over samples_per_ray cosine-weighted directions drawn on the device (irradiance = pi * that)
    pub fn vk_trace_irradiance(scene: *mut vk_scene, params: *const vk_radiance_params, points: *const vk_ray, n_points: u64,
                               rgb_out: *mut f32, stats_out: *mut vk_stats) -> c_int;
    // probe queries (additive symbols of ABI 7): a probe is a vk_ray whose origin is the position (the direction is not read);
    // sh_out[(i * 9 + k) * 3 + c] = the mean of Y_k(u) * L_c(u) over samples_per_ray uniform directions drawn on the device (the
    // radiance's SH coefficient = 4 pi * that).  vk_probe_eval touches no device: mode 0 = radiance along n, 1 = irradiance / pi
    pub fn vk_trace_probes(scene: *mut vk_scene, params: *const vk_radiance_params, probes: *const vk_ray, n_probes: u64,
                           sh_out: *mut f32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_probe_eval(sh27: *const f32, n: *const f32, mode: u32, rgb: *mut f32) -> c_int;
    // shade queries (additive symbols of ABI 7): one bounce of ray_color for (rays[i], hits[i], states[i]); out[i].next and out[i].state
    // feed vk_trace_rays and the next call while out[i].status is VK_SHADE_SCATTERED
    pub fn vk_shade_hits(scene: *mut vk_scene, params: *const vk_shade_params, rays: *const vk_ray, hits: *const vk_hit,
                         states: *const vk_path_state, n: u64, out: *mut vk_shaded, stats_out: *mut vk_stats) -> c_int;
    // path batches (additive symbols of ABI 7): the loop around trace and shade on the device, with a stable compaction per bounce;
    // begin, then step until vk_paths_step_info.live is 0, then results; read and cull between steps; destroy before the scene
    pub fn vk_paths_create(scene: *mut vk_scene, capacity: u64, out: *mut *mut vk_paths) -> c_int;
    pub fn vk_paths_begin(p: *mut vk_paths, params: *const vk_shade_params, rays: *const vk_ray, states: *const vk_path_state, n: u64) -> c_int;
    pub fn vk_paths_step(p: *mut vk_paths, max_bounces: u32, info: *mut vk_paths_step_info) -> c_int;
    pub fn vk_paths_read(p: *mut vk_paths, ids: *mut u32, rays: *mut vk_ray, states: *mut vk_path_state) -> c_int;
    pub fn vk_paths_cull(p: *mut vk_paths, keep: *const u8, scale: *const f32) -> c_int;
    pub fn vk_paths_results(p: *mut vk_paths, states: *mut vk_path_state, status: *mut u32) -> c_int;
    pub fn vk_paths_get_info(p: *mut vk_paths, out: *mut vk_paths_info) -> c_int;
    pub fn vk_paths_destroy(p: *mut vk_paths);
    // the handle's Russian roulette: on the device inside every bounce of vk_paths_step and vk_regen_step; rp null turns it off
    pub fn vk_roulette_set(p: *mut vk_paths, rp: *const vk_roulette_params) -> c_int;
    pub fn vk_roulette_get(p: *mut vk_paths, out: *mut vk_roulette_params, enabled: *mut c_int) -> c_int;
    // films (additive symbols of ABI 7): a frame's sums on the device; emit camera paths into a batch, step the batch until nothing is
    // live, deposit it; resolve(samples_per_pixel) once every (pixel, sample) went through is vk_render's frame; destroy before the scene
    pub fn vk_film_create(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, out: *mut *mut vk_film) -> c_int;
    pub fn vk_film_emit(film: *mut vk_film, batch: *mut vk_paths, win: *const vk_film_window) -> c_int;
    pub fn vk_film_deposit(film: *mut vk_film, batch: *mut vk_paths) -> c_int;
    pub fn vk_film_resolve(film: *mut vk_film, n: u32, rgb_out: *mut f32) -> c_int;
    pub fn vk_film_reset(film: *mut vk_film, cam: *const vk_camera) -> c_int;
    pub fn vk_film_get_info(film: *mut vk_film, out: *mut vk_film_info) -> c_int;
    pub fn vk_film_destroy(film: *mut vk_film);
    // regeneration (additive symbols of ABI 7): begin a run of a window of any size through a batch of any capacity, then step until
    // vk_regen_info.live and .remaining are both 0; the retired paths are deposited into the film as they retire
    pub fn vk_regen_begin(film: *mut vk_film, batch: *mut vk_paths, win: *const vk_film_window) -> c_int;
    pub fn vk_regen_step(film: *mut vk_film, batch: *mut vk_paths, max_bounces: u32, info: *mut vk_regen_info) -> c_int;
    pub fn vk_regen_cull(film: *mut vk_film, batch: *mut vk_paths, keep: *const u8, scale: *const f32) -> c_int;
    // a film's error moments and adaptive regeneration (additive symbols of ABI 7): enable before the first emit, then per window
    // vk_adapt_begin, vk_regen_step until the run is finished, vk_adapt_close; ap null keeps the moments and freezes no tile
    pub fn vk_adapt_enable(film: *mut vk_film, ap: *const vk_adaptive_params) -> c_int;
    pub fn vk_adapt_begin(film: *mut vk_film, batch: *mut vk_paths, n_samples: u32) -> c_int;
    pub fn vk_adapt_close(film: *mut vk_film, n_samples: u32, info: *mut vk_adapt_info) -> c_int;
    pub fn vk_adapt_resolve(film: *mut vk_film, rgb_out: *mut f32) -> c_int;
    pub fn vk_adapt_stderr(film: *mut vk_film, out: *mut f32) -> c_int;
    pub fn vk_adapt_tile_samples(film: *mut vk_film, out: *mut u32, info: *mut vk_adaptive_info) -> c_int;
    // reconstruction filters (additive symbols of ABI 7): a finished batch splatted into a filtered frame (box, tent, Mitchell-Netravali);
    // positions: null (the state's pixel and the sample's own jitter) or 2 * started frame coordinates
    pub fn vk_splat_default_params(out: *mut vk_splat_params) -> c_int;
    pub fn vk_splat_create(scene: *mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, sp: *const vk_splat_params, out: *mut *mut vk_splat) -> c_int;
    pub fn vk_splat_deposit(s: *mut vk_splat, batch: *mut vk_paths, positions: *const f32) -> c_int;
    pub fn vk_splat_resolve(s: *mut vk_splat, rgb_out: *mut f32) -> c_int;
    pub fn vk_splat_reset(s: *mut vk_splat) -> c_int;
    pub fn vk_splat_get_info(s: *mut vk_splat, out: *mut vk_splat_info) -> c_int;
    pub fn vk_splat_destroy(s: *mut vk_splat);
    // robust film (additive symbols of ABI 7): a finished batch added to K bucketed sums per pixel, resolved as a plain, trimmed or
    // Gini-trimmed mean of the buckets with the standard error of the kept bucket means; how: null (create's) or another mode / trim
    pub fn vk_robust_default_params(out: *mut vk_robust_params) -> c_int;
    pub fn vk_robust_create(scene: *mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, rp: *const vk_robust_params, out: *mut *mut vk_robust) -> c_int;
    pub fn vk_robust_deposit(s: *mut vk_robust, batch: *mut vk_paths) -> c_int;
    pub fn vk_robust_resolve(s: *mut vk_robust, how: *const vk_robust_params, rgb_out: *mut f32, stderr3_out: *mut f32) -> c_int;
    pub fn vk_robust_reset(s: *mut vk_robust) -> c_int;
    pub fn vk_robust_get_info(s: *mut vk_robust, out: *mut vk_robust_info) -> c_int;
    pub fn vk_robust_destroy(s: *mut vk_robust);
    // light-path layers (additive symbols of ABI 7): vk_paths_step with a tag per path kept behind every bounce, a finished batch added
    // to per-layer sums by the first matching rule, and a layer's (or with VK_LPE_ALL every layer's) resolve; sig, term and share_out may
    // be null
    pub fn vk_lpe_create(scene: *mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, capacity: u64, lp: *const vk_lpe_params, out: *mut *mut vk_lpe) -> c_int;
    pub fn vk_lpe_step(s: *mut vk_lpe, batch: *mut vk_paths, max_bounces: u32, info: *mut vk_paths_step_info) -> c_int;
    pub fn vk_lpe_tags(s: *mut vk_lpe, batch: *mut vk_paths, sig: *mut u32, term: *mut u32) -> c_int;
    pub fn vk_lpe_deposit(s: *mut vk_lpe, batch: *mut vk_paths) -> c_int;
    pub fn vk_lpe_resolve(s: *mut vk_lpe, layer: u32, n: u32, rgb_out: *mut f32, share_out: *mut f32) -> c_int;
    pub fn vk_lpe_reset(s: *mut vk_lpe) -> c_int;
    pub fn vk_lpe_get_info(s: *mut vk_lpe, out: *mut vk_lpe_info) -> c_int;
    pub fn vk_lpe_destroy(s: *mut vk_lpe);
    // display transform (additive symbols of ABI 7): a frame's luminance histogram and metered exposure, and its encoding through a tone
    // curve and a transfer to width * height * 3 bytes, row 0 the top; load_device and encode_device are enqueued on the null stream;
    // solve is host code (bins: 640 words; prev_log2: null for a first meter)
    pub fn vk_tone_default_meter_params(out: *mut vk_tone_meter_params) -> c_int;
    pub fn vk_tone_default_params(out: *mut vk_tone_params) -> c_int;
    pub fn vk_tone_create(scene: *mut vk_scene, width: u32, height: u32, out: *mut *mut vk_tone) -> c_int;
    pub fn vk_tone_load(t: *mut vk_tone, rgb: *const f32) -> c_int;
    pub fn vk_tone_load_device(t: *mut vk_tone, d_rgb: *const c_void) -> c_int;
    pub fn vk_tone_meter(t: *mut vk_tone, mp: *const vk_tone_meter_params, out: *mut vk_tone_meter_info) -> c_int;
    pub fn vk_tone_solve(bins: *const u32, mp: *const vk_tone_meter_params, prev_log2: *const f64, out: *mut vk_tone_meter_info) -> c_int;
    pub fn vk_tone_encode(t: *mut vk_tone, tp: *const vk_tone_params, rgb8_out: *mut u8) -> c_int;
    pub fn vk_tone_encode_device(t: *mut vk_tone, tp: *const vk_tone_params, d_rgb8_out: *mut c_void) -> c_int;
    pub fn vk_tone_reset(t: *mut vk_tone) -> c_int;
    pub fn vk_tone_get_info(t: *mut vk_tone, out: *mut vk_tone_info) -> c_int;
    pub fn vk_tone_destroy(t: *mut vk_tone);
    // non-local means (additive symbols of ABI 7): a frame and its standard error loaded into a handle, filtered by variance-cancelling
    // patch distances; no function takes a stream (the _device calls are enqueued on the null stream)
    pub fn vk_nlm_default_params(out: *mut vk_nlm_params) -> c_int;
    pub fn vk_nlm_create(scene: *mut vk_scene, width: u32, height: u32, out: *mut *mut vk_nlm) -> c_int;
    pub fn vk_nlm_load(h: *mut vk_nlm, color: *const f32, stderr3: *const f32, albedo: *const f32) -> c_int;
    pub fn vk_nlm_load_device(h: *mut vk_nlm, d_color: *const c_void, d_stderr3: *const c_void, d_albedo: *const c_void) -> c_int;
    pub fn vk_nlm_filter(h: *mut vk_nlm, p: *const vk_nlm_params, rgb_out: *mut f32, stderr3_out: *mut f32) -> c_int;
    pub fn vk_nlm_filter_device(h: *mut vk_nlm, p: *const vk_nlm_params, d_rgb_out: *mut c_void, d_stderr3_out: *mut c_void) -> c_int;
    pub fn vk_nlm_reset(h: *mut vk_nlm) -> c_int;
    pub fn vk_nlm_get_info(h: *mut vk_nlm, out: *mut vk_nlm_info) -> c_int;
    pub fn vk_nlm_destroy(h: *mut vk_nlm);
    // glare (additive symbols of ABI 7): the share `strength` of a frame's bright part spread over a pyramid of halved images, in front
    // of the display transform; no function takes a stream (the _device call is enqueued on the null stream); out may be in
    pub fn vk_glare_default_params(out: *mut vk_glare_params) -> c_int;
    pub fn vk_glare_create(scene: *mut vk_scene, width: u32, height: u32, out: *mut *mut vk_glare) -> c_int;
    pub fn vk_glare_apply(g: *mut vk_glare, p: *const vk_glare_params, rgb_in: *const f32, rgb_out: *mut f32) -> c_int;
    pub fn vk_glare_apply_device(g: *mut vk_glare, p: *const vk_glare_params, d_rgb_in: *const c_void, d_rgb_out: *mut c_void) -> c_int;
    pub fn vk_glare_get_info(g: *mut vk_glare, out: *mut vk_glare_info) -> c_int;
    pub fn vk_glare_destroy(g: *mut vk_glare);
    // point-spread function (additive symbols of ABI 7): the share `strength` of a frame's bright part convolved with a caller's K x K x 3
    // kernel in the Fourier domain, between vk_glare and vk_tone; no function takes a stream
    pub fn vk_psf_default_params(out: *mut vk_psf_params) -> c_int;
    pub fn vk_psf_star(K: u32, streaks: u32, rotation: f32, sharpness: f32, chroma: f32, out: *mut f32) -> c_int;
    pub fn vk_psf_create(scene: *mut vk_scene, width: u32, height: u32, kmax: u32, out: *mut *mut vk_psf) -> c_int;
    pub fn vk_psf_load(h: *mut vk_psf, K: u32, kernel: *const f32) -> c_int;
    pub fn vk_psf_load_device(h: *mut vk_psf, K: u32, d_kernel: *const c_void) -> c_int;
    pub fn vk_psf_apply(h: *mut vk_psf, p: *const vk_psf_params, rgb_in: *const f32, rgb_out: *mut f32) -> c_int;
    pub fn vk_psf_apply_device(h: *mut vk_psf, p: *const vk_psf_params, d_rgb_in: *const c_void, d_rgb_out: *mut c_void) -> c_int;
    pub fn vk_psf_reset(h: *mut vk_psf) -> c_int;
    pub fn vk_psf_get_info(h: *mut vk_psf, out: *mut vk_psf_info) -> c_int;
    pub fn vk_psf_destroy(h: *mut vk_psf);
    // guided upsampling (additive symbols of ABI 7): a w x h frame and its stderr3 to W x H along the edges of albedo, normal and depth
    // given at both sizes; every image but color_lo and rgb_out may be null; no function takes a stream (the _device calls are enqueued
    // on the null stream)
    pub fn vk_upsample_default_params(out: *mut vk_upsample_params) -> c_int;
    pub fn vk_upsample_create(scene: *mut vk_scene, w: u32, h: u32, width_hi: u32, height_hi: u32, out: *mut *mut vk_upsample) -> c_int;
    pub fn vk_upsample_load(u: *mut vk_upsample, color_lo: *const f32, stderr3_lo: *const f32, albedo_lo: *const f32, normal_lo: *const f32, depth_lo: *const f32) -> c_int;
    pub fn vk_upsample_load_device(u: *mut vk_upsample, d_color_lo: *const c_void, d_stderr3_lo: *const c_void, d_albedo_lo: *const c_void, d_normal_lo: *const c_void, d_depth_lo: *const c_void) -> c_int;
    pub fn vk_upsample_apply(u: *mut vk_upsample, p: *const vk_upsample_params, albedo_hi: *const f32, normal_hi: *const f32, depth_hi: *const f32, rgb_out: *mut f32, stderr3_out: *mut f32) -> c_int;
    pub fn vk_upsample_apply_device(u: *mut vk_upsample, p: *const vk_upsample_params, d_albedo_hi: *const c_void, d_normal_hi: *const c_void, d_depth_hi: *const c_void, d_rgb_out: *mut c_void, d_stderr3_out: *mut c_void) -> c_int;
    pub fn vk_upsample_reset(u: *mut vk_upsample) -> c_int;
    pub fn vk_upsample_get_info(u: *mut vk_upsample, out: *mut vk_upsample_info) -> c_int;
    pub fn vk_upsample_destroy(u: *mut vk_upsample);
    // ID mattes (additive symbols of ABI 7): a ranked table of object or material ids per pixel, ids / counts ranks words per pixel,
    // overflow one (may be null); merge and mask are host code
    pub fn vk_matte_default_params(out: *mut vk_matte_params) -> c_int;
    pub fn vk_render_mattes(scene: *mut vk_scene, cam: *const vk_camera, params: *const vk_render_params, first_sample: u32,
                            mp: *const vk_matte_params, ids: *mut u32, counts: *mut u32, overflow: *mut u32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_matte_merge(ranks: u32, n_pixels: u64, ids: *mut u32, counts: *mut u32, overflow: *mut u32, ids_b: *const u32,
                          counts_b: *const u32, overflow_b: *const u32) -> c_int;
    pub fn vk_matte_mask(ranks: u32, n_pixels: u64, ids: *const u32, counts: *const u32, n_samples: u32, want: *const u32, n_want: u32,
                         mask_out: *mut f32) -> c_int;
    // the denoiser (additive symbols of ABI 7): color and out are required, each of stderr3 / albedo / normal / depth may be null
    pub fn vk_denoise_default_params(width: u32, height: u32, out: *mut vk_denoise_params) -> c_int;
    pub fn vk_denoise(scene: *mut vk_scene, dp: *const vk_denoise_params, color: *const f32, stderr3: *const f32, albedo: *const f32,
                      normal: *const f32, depth: *const f32, out: *mut f32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_denoise_device(scene: *mut vk_scene, dp: *const vk_denoise_params, d_color: *const c_void, d_stderr3: *const c_void,
                             d_albedo: *const c_void, d_normal: *const c_void, d_depth: *const c_void, d_out: *mut c_void,
                             hip_stream: *mut c_void) -> c_int;
    pub fn vk_progress_stderr_device(pr: *mut vk_progress, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    // temporal accumulation (additive symbols of ABI 7): color, normal, depth, out_color and cam are required; stderr3, albedo,
    // out_stderr3 and out_history may be null (out_stderr3 needs stderr3)
    pub fn vk_temporal_default_params(width: u32, height: u32, out: *mut vk_temporal_params) -> c_int;
    pub fn vk_temporal_create(scene: *mut vk_scene, tp: *const vk_temporal_params, out: *mut *mut vk_temporal) -> c_int;
    pub fn vk_temporal_accumulate(t: *mut vk_temporal, cam: *const vk_camera, color: *const f32, stderr3: *const f32, albedo: *const f32,
                                  normal: *const f32, depth: *const f32, out_color: *mut f32, out_stderr3: *mut f32,
                                  out_history: *mut f32, stats_out: *mut vk_stats) -> c_int;
    pub fn vk_temporal_accumulate_device(t: *mut vk_temporal, cam: *const vk_camera, d_color: *const c_void, d_stderr3: *const c_void,
                                         d_albedo: *const c_void, d_normal: *const c_void, d_depth: *const c_void,
                                         d_out_color: *mut c_void, d_out_stderr3: *mut c_void, d_out_history: *mut c_void,
                                         hip_stream: *mut c_void) -> c_int;
    pub fn vk_temporal_reset(t: *mut vk_temporal) -> c_int;
    pub fn vk_temporal_get_info(t: *mut vk_temporal, out: *mut vk_temporal_info) -> c_int;
    pub fn vk_temporal_destroy(t: *mut vk_temporal);
}

/// What `flatten()` pushes into (flatten.rs).  One record per Arc; shared Arcs are de-duplicated
/// by pointer identity so a light that is both in `world` and in `lights` flattens once.
#[derive(Default)]
pub struct FlatBuilder {
    pub bvh: Vec<vk_bvh_node>, pub spheres: Vec<vk_sphere>, pub moving_spheres: Vec<vk_moving_sphere>, pub rects: Vec<vk_rect>,
    pub lists: Vec<vk_list>, pub list_items: Vec<vk_ref>, pub media: Vec<vk_medium>, pub translates: Vec<vk_translate>,
    pub rotates: Vec<vk_rotate>, pub materials: Vec<vk_material>, pub textures: Vec<vk_texture>, pub images: Vec<vk_image>,
    pub perlins: Vec<vk_perlin>, pub lights: Vec<vk_ref>, pub world: vk_ref,
    pub seen: std::collections::HashMap<usize, u32>,
}

impl FlatBuilder {
    pub fn desc(&self) -> vk_scene_desc {
        vk_scene_desc {
            abi_version: VK_ABI_VERSION,
            n_bvh: self.bvh.len() as u32, bvh: self.bvh.as_ptr(),
            n_spheres: self.spheres.len() as u32, spheres: self.spheres.as_ptr(),
            n_moving_spheres: self.moving_spheres.len() as u32, moving_spheres: self.moving_spheres.as_ptr(),
            n_rects: self.rects.len() as u32, rects: self.rects.as_ptr(),
            n_lists: self.lists.len() as u32, lists: self.lists.as_ptr(),
            n_list_items: self.list_items.len() as u32, list_items: self.list_items.as_ptr(),
            n_media: self.media.len() as u32, media: self.media.as_ptr(),
            n_translates: self.translates.len() as u32, translates: self.translates.as_ptr(),
            n_rotates: self.rotates.len() as u32, rotates: self.rotates.as_ptr(),
            n_materials: self.materials.len() as u32, materials: self.materials.as_ptr(),
            n_textures: self.textures.len() as u32, textures: self.textures.as_ptr(),
            n_images: self.images.len() as u32, images: self.images.as_ptr(),
            n_perlins: self.perlins.len() as u32, perlins: self.perlins.as_ptr(),
            world: self.world, n_lights: self.lights.len() as u32, lights: self.lights.as_ptr(), flags: 0,
        }
    }
}

/// Owns the uploaded scene; `render` is the drop-in for the closure at main.rs:181-198.
pub struct GpuScene { handle: *mut vk_scene }

fn check(status: c_int) -> Result<(), std::io::Error> {
    if status == 0 { return Ok(()); }
    let msg = unsafe { CStr::from_ptr(vk_last_error()) }.to_string_lossy().into_owned();
    Err(std::io::Error::new(std::io::ErrorKind::Other, format!("vecchio_amd status {}: {}", status, msg)))
}

impl GpuScene {
    pub fn new(fb: &FlatBuilder, device: i32) -> Result<GpuScene, std::io::Error> {
        let mut h: *mut vk_scene = std::ptr::null_mut();
        let d = fb.desc();
        check(unsafe { vk_scene_create(&d, device, &mut h) })?;
        Ok(GpuScene { handle: h })
    }
    /// One handle over every listed GPU: `render` then deals the tiles over them and gathers on devices[0]
    /// (what `main()`'s single-threaded frame loop, main.rs:176, calls on an 8-GPU node).
    pub fn new_multi(fb: &FlatBuilder, devices: &[i32]) -> Result<GpuScene, std::io::Error> {
        let mut h: *mut vk_scene = std::ptr::null_mut();
        let d = fb.desc();
        check(unsafe { vk_scene_create_multi(&d, devices.as_ptr(), devices.len() as c_int, &mut h) })?;
        Ok(GpuScene { handle: h })
    }
    /// `pixels`: width*height Vec3 (#[repr(C)] added to vec3.rs:3-8), y = 0 bottom row as in main.rs:182-183.
    pub fn render(&self, cam: &vk_camera, params: &vk_render_params, pixels: &mut [[f32; 3]]) -> Result<vk_stats, std::io::Error> {
        assert_eq!(pixels.len(), (params.width * params.height) as usize);
        let mut st = vk_stats::default();
        check(unsafe { vk_render(self.handle, cam, params, pixels.as_mut_ptr() as *mut f32, &mut st) })?;
        Ok(st)
    }
}
impl Drop for GpuScene { fn drop(&mut self) { unsafe { vk_scene_destroy(self.handle) } } }

/// One frame accumulated over sample windows (vk_progress_*): `step` renders the next `n` samples per pixel and leaves the running mean
/// in `pixels` — bit for bit what `GpuScene::render` gives at that many samples.  Borrows the scene: it is dropped before it.
pub struct GpuProgress<'a> { handle: *mut vk_progress, _scene: &'a GpuScene }

impl GpuScene {
    /// `params.samples_per_pixel` is the frame's budget; `with_stderr` keeps the error moments for `stderr`.
    pub fn progress(&self, cam: &vk_camera, params: &vk_render_params, with_stderr: bool) -> Result<GpuProgress<'_>, std::io::Error> {
        let mut h: *mut vk_progress = std::ptr::null_mut();
        check(unsafe { vk_progress_create(self.handle, cam, params, if with_stderr { VK_PROGRESS_STDERR } else { 0 }, &mut h) })?;
        Ok(GpuProgress { handle: h, _scene: self })
    }
}

impl<'a> GpuProgress<'a> {
    pub fn step(&mut self, n: u32, pixels: &mut [[f32; 3]]) -> Result<vk_stats, std::io::Error> {
        let mut st = vk_stats::default();
        check(unsafe { vk_progress_step(self.handle, n, pixels.as_mut_ptr() as *mut c_void, &mut st) })?;
        Ok(st)
    }
    /// per-component standard error of the running mean (batch means over the steps; needs `with_stderr` and two steps)
    pub fn stderr(&mut self, out: &mut [[f32; 3]]) -> Result<(), std::io::Error> {
        check(unsafe { vk_progress_stderr(self.handle, out.as_mut_ptr() as *mut f32) })
    }
    pub fn info(&mut self) -> Result<vk_progress_info, std::io::Error> {
        let mut i = vk_progress_info::default();
        check(unsafe { vk_progress_get_info(self.handle, &mut i) })?;
        Ok(i)
    }
    pub fn reset(&mut self, cam: Option<&vk_camera>) -> Result<(), std::io::Error> {
        check(unsafe { vk_progress_reset(self.handle, cam.map_or(std::ptr::null(), |c| c as *const vk_camera)) })
    }
    /// adaptive sampling: converged tiles stop (needs `with_stderr`; before the first step since create / reset)
    pub fn set_adaptive(&mut self, ap: &vk_adaptive_params) -> Result<(), std::io::Error> {
        check(unsafe { vk_progress_set_adaptive(self.handle, ap) })
    }
    /// samples per 8x8 tile (`tiles_x * tiles_y`, tile row 0 at the bottom; 0 outside the partition) and the active count
    pub fn tile_samples(&mut self, out: &mut [u32]) -> Result<vk_adaptive_info, std::io::Error> {
        let mut i = vk_adaptive_info::default();
        check(unsafe { vk_progress_tile_samples(self.handle, out.as_mut_ptr(), &mut i) })?;
        Ok(i)
    }
}
impl<'a> Drop for GpuProgress<'a> { fn drop(&mut self) { unsafe { vk_progress_destroy(self.handle) } } }
