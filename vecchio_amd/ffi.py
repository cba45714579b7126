"""ctypes mirror of include/vecchio_amd.h and vecchio_amd/host/host_api.h.

Plumbing only: the product is libvecchio_amd.so (HIP megakernel behind the C ABI) and
libvecchio_host.so (C++ stand-in for the reference's Rust host side).  There is no CPU
fallback here: `load_device_lib()` raises if the HIP library is missing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
ASSETS_DIR = os.path.join(os.path.dirname(_HERE), "tests", "golden", "assets")

VK_ABI_VERSION = 7
VK_PROBE_COEFFS = 9
VK_OK, VK_ERR_BAD_ARG, VK_ERR_UNSUPPORTED, VK_ERR_HIP, VK_ERR_NO_DEVICE, VK_ERR_OOM = range(6)

(VK_KIND_NONE, VK_KIND_BVH, VK_KIND_SPHERE, VK_KIND_MOVING_SPHERE, VK_KIND_RECT, VK_KIND_LIST,
 VK_KIND_MEDIUM, VK_KIND_TRANSLATE, VK_KIND_ROTATE) = range(9)
VK_REF_FLIP = 0x08000000
VK_REF_INDEX_MASK = 0x07FFFFFF

(VK_MAT_LAMBERTIAN, VK_MAT_METAL, VK_MAT_DIELECTRIC, VK_MAT_DIFFUSE_LIGHT, VK_MAT_ISOTROPIC,
 VK_MAT_SPEC_DIFFUSE) = range(6)
VK_TEX_SOLID, VK_TEX_CHECKER, VK_TEX_IMAGE, VK_TEX_NOISE = range(4)
VK_MAX_CHECKER_DEPTH, VK_MAX_SPEC_DIFFUSE_DEPTH = 15, 8      # deepest nesting the device resolves (include/vecchio_amd.h)
VK_INTEGRATOR_PDF, VK_INTEGRATOR_SCATTER = 0, 1
VK_BACKGROUND_SOLID, VK_BACKGROUND_SKY = 0, 1
VK_OUTPUT_F32, VK_OUTPUT_RGB8 = 0, 1
VK_SCENE_FAST_ACCEL = 1
VK_SCENE_REFERENCE_TREE = 2
VK_SCENE_EMPIRICAL_TREES = 4
VK_SCENE_RCCL_GATHER = 8
VK_PROGRESS_STDERR = 1


def make_ref(kind, index, flip=False):
    return (kind << 28) | (index & VK_REF_INDEX_MASK) | (VK_REF_FLIP if flip else 0)


F3 = C.c_float * 3


class BvhNode(C.Structure):
    _fields_ = [("bb_min", F3), ("bb_max", F3), ("left", C.c_uint32), ("right", C.c_uint32)]


class Sphere(C.Structure):
    _fields_ = [("center", F3), ("radius", C.c_float), ("material", C.c_uint32)]


class MovingSphere(C.Structure):
    _fields_ = [("center0", F3), ("center1", F3), ("time0", C.c_float), ("time1", C.c_float),
                ("radius", C.c_float), ("material", C.c_uint32)]


class Rect(C.Structure):
    _fields_ = [("c0", C.c_float), ("c1", C.c_float), ("d0", C.c_float), ("d1", C.c_float), ("k", C.c_float),
                ("axis0", C.c_uint8), ("axis1", C.c_uint8), ("axis2", C.c_uint8), ("_pad", C.c_uint8),
                ("material", C.c_uint32)]


class List(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32)]


class Medium(C.Structure):
    _fields_ = [("boundary", C.c_uint32), ("neg_inv_density", C.c_float), ("material", C.c_uint32)]


class Translate(C.Structure):
    _fields_ = [("child", C.c_uint32), ("offset", F3)]


class Rotate(C.Structure):
    _fields_ = [("child", C.c_uint32), ("axis", C.c_uint32), ("sin_theta", C.c_float), ("cos_theta", C.c_float)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("texture", C.c_uint32), ("param", C.c_float), ("a", C.c_uint32), ("b", C.c_uint32)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("color", F3), ("a", C.c_uint32), ("b", C.c_uint32), ("scale", C.c_float)]


class Image(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_uint8))]


class Perlin(C.Structure):
    _fields_ = [("ranvec", (C.c_float * 3) * 256), ("perm_x", C.c_uint32 * 256), ("perm_y", C.c_uint32 * 256),
                ("perm_z", C.c_uint32 * 256)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_bvh", C.c_uint32), ("bvh", C.POINTER(BvhNode)),
        ("n_spheres", C.c_uint32), ("spheres", C.POINTER(Sphere)),
        ("n_moving_spheres", C.c_uint32), ("moving_spheres", C.POINTER(MovingSphere)),
        ("n_rects", C.c_uint32), ("rects", C.POINTER(Rect)),
        ("n_lists", C.c_uint32), ("lists", C.POINTER(List)),
        ("n_list_items", C.c_uint32), ("list_items", C.POINTER(C.c_uint32)),
        ("n_media", C.c_uint32), ("media", C.POINTER(Medium)),
        ("n_translates", C.c_uint32), ("translates", C.POINTER(Translate)),
        ("n_rotates", C.c_uint32), ("rotates", C.POINTER(Rotate)),
        ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
        ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
        ("n_images", C.c_uint32), ("images", C.POINTER(Image)),
        ("n_perlins", C.c_uint32), ("perlins", C.POINTER(Perlin)),
        ("world", C.c_uint32),
        ("n_lights", C.c_uint32), ("lights", C.POINTER(C.c_uint32)),
        ("flags", C.c_uint32),
    ]


class Camera(C.Structure):
    _fields_ = [("origin", F3), ("lower_left_corner", F3), ("horizontal", F3), ("vertical", F3),
                ("u", F3), ("v", F3), ("w", F3), ("lens_radius", C.c_float), ("time0", C.c_float), ("time1", C.c_float)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_pixel", C.c_uint32),
                ("max_depth", C.c_uint32), ("seed", C.c_uint64), ("integrator", C.c_uint32),
                ("background", C.c_uint32), ("background_color", F3), ("tile_rank", C.c_uint32),
                ("tile_world", C.c_uint32), ("output_format", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("seconds", C.c_double), ("kernel_ms", C.c_double),
                ("kernel_launches", C.c_uint32), ("scene_in_lds", C.c_uint32), ("clamped_samples", C.c_uint64)]


class SceneInfo(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("n_prims", C.c_uint32), ("n_instances", C.c_uint32),
                ("device_bytes", C.c_uint64), ("lds_bytes", C.c_uint32), ("features", C.c_uint32), ("tree", C.c_uint32),
                ("tree_suspended_frames", C.c_uint32), ("gather", C.c_uint32)]


class PartInfo(C.Structure):
    _fields_ = [("n_parts", C.c_uint32), ("device", C.c_int32), ("name", C.c_char * 64), ("pci_bus_id", C.c_char * 32),
                ("can_access_landing_device", C.c_uint32), ("kernel_ms", C.c_double)]


class ProgressInfo(C.Structure):
    _fields_ = [("samples_done", C.c_uint32), ("samples_budget", C.c_uint32), ("steps", C.c_uint32), ("flags", C.c_uint32),
                ("clamped_samples", C.c_uint64)]


class AdaptiveParams(C.Structure):
    """vk_adaptive_params (vk_progress_set_adaptive)"""
    _fields_ = [("abs_tol", C.c_float), ("rel_tol", C.c_float), ("min_samples", C.c_uint32), ("min_steps", C.c_uint32)]


class AdaptiveInfo(C.Structure):
    """vk_adaptive_info (vk_progress_tile_samples)"""
    _fields_ = [("tiles_total", C.c_uint32), ("tiles_active", C.c_uint32), ("samples_rendered", C.c_uint64)]


class Ray(C.Structure):
    """vk_ray (vk_trace_rays): tmax = inf for the reference's own call"""
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("direction", C.c_float * 3), ("time", C.c_float)]


class Hit(C.Structure):
    """vk_hit (vk_trace_rays)"""
    _fields_ = [("p", C.c_float * 3), ("t", C.c_float), ("normal", C.c_float * 3), ("u", C.c_float), ("v", C.c_float),
                ("hit", C.c_uint32), ("front", C.c_uint32), ("material", C.c_uint32), ("object", C.c_uint32), ("medium", C.c_uint32),
                ("_pad", C.c_uint32 * 2)]


class TraceParams(C.Structure):
    """vk_trace_params (vk_trace_rays)"""
    _fields_ = [("seed", C.c_uint64), ("first_index", C.c_uint64), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


VK_RAY_TMIN = 0.001


class RadianceParams(C.Structure):
    """vk_radiance_params (vk_trace_radiance)"""
    _fields_ = [("seed", C.c_uint64), ("first_index", C.c_uint64), ("samples_per_ray", C.c_uint32), ("first_sample", C.c_uint32),
                ("max_depth", C.c_uint32), ("integrator", C.c_uint32), ("background", C.c_uint32), ("background_color", F3),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class PathState(C.Structure):
    """vk_path_state (vk_shade_hits): a fresh path has thr (1,1,1), depth 1, acc (0,0,0), counter 0"""
    _fields_ = [("thr", C.c_float * 3), ("depth", C.c_uint32), ("acc", C.c_float * 3), ("counter", C.c_uint32), ("seed", C.c_uint64),
                ("pixel", C.c_uint32), ("sample", C.c_uint32)]


class Shaded(C.Structure):
    """vk_shaded (vk_shade_hits)"""
    _fields_ = [("next", Ray), ("state", PathState), ("status", C.c_uint32), ("lobe", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class ShadeParams(C.Structure):
    """vk_shade_params (vk_shade_hits)"""
    _fields_ = [("max_depth", C.c_uint32), ("integrator", C.c_uint32), ("background", C.c_uint32), ("background_color", F3),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


VK_SHADE_MISS, VK_SHADE_SCATTERED, VK_SHADE_ENDED, VK_SHADE_BAD_HIT = range(4)
VK_PATHS_LIVE, VK_PATHS_CULLED = 1, 4


class PathsInfo(C.Structure):
    """vk_paths_info (vk_paths_get_info)"""
    _fields_ = [("capacity", C.c_uint64), ("started", C.c_uint64), ("live", C.c_uint64), ("retired", C.c_uint64 * 5), ("bounces", C.c_uint32),
                ("_pad", C.c_uint32)]


class PathsStepInfo(C.Structure):
    """vk_paths_step_info (vk_paths_step)"""
    _fields_ = [("traced", C.c_uint64), ("live", C.c_uint64), ("missed", C.c_uint64), ("ended", C.c_uint64), ("bad", C.c_uint64),
                ("bounces", C.c_uint32), ("kernel_launches", C.c_uint32), ("kernel_ms", C.c_double), ("seconds", C.c_double)]


class RouletteParams(C.Structure):
    """vk_roulette_params (vk_roulette_set)"""
    _fields_ = [("first_depth", C.c_uint32), ("q_min", C.c_float), ("q_max", C.c_float), ("flags", C.c_uint32)]


class FilmWindow(C.Structure):
    """vk_film_window (vk_film_emit)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("first_sample", C.c_uint32),
                ("n_samples", C.c_uint32)]


class FilmInfo(C.Structure):
    """vk_film_info (vk_film_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_pixel", C.c_uint32), ("_pad", C.c_uint32),
                ("emitted", C.c_uint64), ("deposited", C.c_uint64), ("dropped", C.c_uint64), ("clamped", C.c_uint64), ("skipped", C.c_uint64),
                ("deposits", C.c_uint64)]


VK_DEBUG_FILM_DEPOSIT_PLAIN, VK_DEBUG_FILM_DEPOSIT_RUNS = 0, 1


class SplatParams(C.Structure):
    """vk_splat_params (vk_splat_create)"""
    _fields_ = [("filter", C.c_uint32), ("radius", C.c_float), ("b", C.c_float), ("c", C.c_float)]


class SplatInfo(C.Structure):
    """vk_splat_info (vk_splat_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_pixel", C.c_uint32), ("filter", C.c_uint32),
                ("deposited", C.c_uint64), ("dropped", C.c_uint64), ("clamped", C.c_uint64), ("skipped", C.c_uint64),
                ("deposits", C.c_uint64), ("contributions", C.c_uint64)]


VK_SPLAT_BOX, VK_SPLAT_TENT, VK_SPLAT_MITCHELL = 0, 1, 2
VK_DEBUG_SPLAT_FORM_DEFAULT, VK_DEBUG_SPLAT_FORM_PLAIN, VK_DEBUG_SPLAT_FORM_TILED = 0, 1, 2


class MatteParams(C.Structure):
    """vk_matte_params (vk_render_mattes)"""
    _fields_ = [("kind", C.c_uint32), ("ranks", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


VK_MATTE_OBJECT, VK_MATTE_MATERIAL = 0, 1
VK_MATTE_BACKGROUND = 0xFFFFFFFF
VK_MATTE_MAX_RANKS = 8


class RobustParams(C.Structure):
    """vk_robust_params (vk_robust_create, vk_robust_resolve)"""
    _fields_ = [("buckets", C.c_uint32), ("mode", C.c_uint32), ("trim", C.c_uint32), ("_pad", C.c_uint32)]


class RobustInfo(C.Structure):
    """vk_robust_info (vk_robust_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_pixel", C.c_uint32), ("buckets", C.c_uint32),
                ("deposited", C.c_uint64), ("dropped", C.c_uint64), ("clamped", C.c_uint64), ("skipped", C.c_uint64),
                ("deposits", C.c_uint64), ("_reserved", C.c_uint64)]


VK_ROBUST_MEAN, VK_ROBUST_TRIM, VK_ROBUST_GINI = 0, 1, 2


class LpeRule(C.Structure):
    """vk_lpe_rule (vk_lpe_create)"""
    _fields_ = [("sig_mask", C.c_uint32), ("sig_value", C.c_uint32), ("status_mask", C.c_uint32), ("depth_min", C.c_uint32),
                ("depth_max", C.c_uint32), ("emitter", C.c_uint32), ("layer", C.c_uint32), ("_pad", C.c_uint32)]


class LpeParams(C.Structure):
    """vk_lpe_params (vk_lpe_create)"""
    _fields_ = [("n_layers", C.c_uint32), ("rest_layer", C.c_uint32), ("n_rules", C.c_uint32), ("_pad", C.c_uint32),
                ("rules", C.POINTER(LpeRule))]


class LpeInfo(C.Structure):
    """vk_lpe_info (vk_lpe_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_pixel", C.c_uint32), ("n_layers", C.c_uint32),
                ("rest_layer", C.c_uint32), ("n_rules", C.c_uint32), ("capacity", C.c_uint64),
                ("deposited", C.c_uint64), ("dropped", C.c_uint64), ("clamped", C.c_uint64), ("skipped", C.c_uint64),
                ("deposits", C.c_uint64), ("recorded", C.c_uint64)]


VK_LPE_SKY, VK_LPE_EMIT, VK_LPE_OTHER, VK_LPE_BAD = 1, 5, 14, 15
VK_LPE_ALL = 0xFFFFFFFF


class ToneMeterParams(C.Structure):
    """vk_tone_meter_params (vk_tone_meter, vk_tone_solve)"""
    _fields_ = [("key", C.c_float), ("low_fraction", C.c_float), ("high_fraction", C.c_float), ("blend", C.c_float),
                ("min_log2", C.c_float), ("max_log2", C.c_float), ("_pad", C.c_uint32 * 2)]


class ToneMeterInfo(C.Structure):
    """vk_tone_meter_info (vk_tone_meter, vk_tone_solve)"""
    _fields_ = [("log2_target", C.c_double), ("log2_used", C.c_double), ("binned", C.c_uint64), ("below", C.c_uint64),
                ("above", C.c_uint64), ("nonfinite", C.c_uint64), ("exposure", C.c_float), ("flags", C.c_uint32)]


class ToneParams(C.Structure):
    """vk_tone_params (vk_tone_encode, vk_tone_encode_device)"""
    _fields_ = [("curve", C.c_uint32), ("transfer", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32),
                ("exposure", C.c_float), ("white", C.c_float), ("seed", C.c_uint64)]


class ToneInfo(C.Structure):
    """vk_tone_info (vk_tone_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("loads", C.c_uint64), ("meters", C.c_uint64), ("encodes", C.c_uint64),
                ("exposure", C.c_float), ("metered", C.c_uint32), ("log2_used", C.c_double)]


VK_TONE_CLAMP, VK_TONE_REINHARD, VK_TONE_HABLE, VK_TONE_ACES = 0, 1, 2, 3
VK_TONE_TRANSFER_REFERENCE, VK_TONE_TRANSFER_SRGB, VK_TONE_TRANSFER_GAMMA22 = 0, 1, 2
VK_TONE_USE_METERED, VK_TONE_DITHER = 1, 2
VK_TONE_METER_EMPTY = 1
VK_TONE_FORM_LDS, VK_TONE_FORM_PLAIN = 0, 1


class NlmParams(C.Structure):
    """vk_nlm_params (vk_nlm_filter, vk_nlm_filter_device)"""
    _fields_ = [("search_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float),
                ("albedo_floor", C.c_float), ("flags", C.c_uint32)]


class NlmInfo(C.Structure):
    """vk_nlm_info (vk_nlm_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("loaded", C.c_uint32), ("has_albedo", C.c_uint32),
                ("loads", C.c_uint64), ("filters", C.c_uint64), ("last_launches", C.c_uint32), ("last_form", C.c_uint32),
                ("last_kernel_ms", C.c_double), ("scratch_bytes", C.c_uint64)]


VK_NLM_FORM_AUTO, VK_NLM_FORM_PLAIN, VK_NLM_FORM_TILED = 0, 1, 2


class GlareParams(C.Structure):
    """vk_glare_params (vk_glare_apply, vk_glare_apply_device)"""
    _fields_ = [("levels", C.c_uint32), ("strength", C.c_float), ("falloff", C.c_float), ("threshold", C.c_float),
                ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class GlareInfo(C.Structure):
    """vk_glare_info (vk_glare_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("applies", C.c_uint64), ("last_levels", C.c_uint32),
                ("last_form", C.c_uint32), ("last_launches", C.c_uint32), ("_pad", C.c_uint32), ("last_kernel_ms", C.c_double),
                ("scratch_bytes", C.c_uint64)]


VK_GLARE_FORM_AUTO, VK_GLARE_FORM_PLAIN, VK_GLARE_FORM_FUSED = 0, 1, 2


class PsfParams(C.Structure):
    """vk_psf_params (vk_psf_apply, vk_psf_apply_device)"""
    _fields_ = [("strength", C.c_float), ("threshold", C.c_float), ("form", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class PsfInfo(C.Structure):
    """vk_psf_info (vk_psf_get_info)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("K", C.c_uint32), ("Px", C.c_uint32), ("Py", C.c_uint32),
                ("kmax", C.c_uint32), ("last_form", C.c_uint32), ("last_launches", C.c_uint32), ("loads", C.c_uint64),
                ("applies", C.c_uint64), ("last_kernel_ms", C.c_double), ("scratch_bytes", C.c_uint64)]


VK_PSF_FORM_AUTO, VK_PSF_FORM_PLAIN, VK_PSF_FORM_LDS = 0, 1, 2


class UpsampleParams(C.Structure):
    """vk_upsample_params (vk_upsample_apply, vk_upsample_apply_device)"""
    _fields_ = [("sigma_z", C.c_float), ("normal_squarings", C.c_uint32), ("albedo_floor", C.c_float), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


class UpsampleInfo(C.Structure):
    """vk_upsample_info (vk_upsample_get_info)"""
    _fields_ = [("width_lo", C.c_uint32), ("height_lo", C.c_uint32), ("width_hi", C.c_uint32), ("height_hi", C.c_uint32),
                ("loaded", C.c_uint32), ("guides", C.c_uint32), ("loads", C.c_uint64), ("applies", C.c_uint64),
                ("last_form", C.c_uint32), ("last_launches", C.c_uint32), ("last_kernel_ms", C.c_double),
                ("scratch_bytes", C.c_uint64), ("fallback_pixels", C.c_uint64), ("empty_pixels", C.c_uint64)]


VK_UPSAMPLE_FORM_AUTO, VK_UPSAMPLE_FORM_PLAIN, VK_UPSAMPLE_FORM_TILED = 0, 1, 2
VK_UPSAMPLE_HAS_STDERR, VK_UPSAMPLE_HAS_ALBEDO, VK_UPSAMPLE_HAS_NORMAL, VK_UPSAMPLE_HAS_DEPTH = 1, 2, 4, 8


class RegenInfo(C.Structure):
    """vk_regen_info (vk_regen_step)"""
    _fields_ = [("traced", C.c_uint64), ("live", C.c_uint64), ("remaining", C.c_uint64), ("emitted", C.c_uint64), ("missed", C.c_uint64),
                ("ended", C.c_uint64), ("bad", C.c_uint64), ("bounces", C.c_uint32), ("kernel_launches", C.c_uint32),
                ("kernel_ms", C.c_double), ("seconds", C.c_double)]


class AdaptInfo(C.Structure):
    """vk_adapt_info (vk_adapt_close)"""
    _fields_ = [("samples_done", C.c_uint32), ("steps", C.c_uint32), ("tiles_total", C.c_uint32), ("tiles_active", C.c_uint32),
                ("pixels_active", C.c_uint64), ("samples_rendered", C.c_uint64)]


class DebugStreamKey(C.Structure):
    """vk_debug_stream_key of include/vecchio_amd_debug.h (vk_debug_trace_radiance_samples)"""
    _fields_ = [("seed", C.c_uint64), ("pixel", C.c_uint32), ("sample", C.c_uint32), ("ctr", C.c_uint32), ("_pad", C.c_uint32)]


class GuideParams(C.Structure):
    """vk_guide_params (vk_render_guides)"""
    _fields_ = [("max_bounces", C.c_uint32), ("fuzz_max", C.c_float), ("flags", C.c_uint32)]


class DenoiseParams(C.Structure):
    """vk_denoise_params (vk_denoise)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32), ("normal_squarings", C.c_uint32),
                ("sigma_l", C.c_float), ("sigma_z", C.c_float), ("albedo_floor", C.c_float), ("flags", C.c_uint32)]


class TemporalParams(C.Structure):
    """vk_temporal_params (vk_temporal_create)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_history", C.c_uint32), ("depth_tol", C.c_float),
                ("normal_cos_min", C.c_float), ("albedo_floor", C.c_float), ("flags", C.c_uint32)]


class TemporalInfo(C.Structure):
    """vk_temporal_info (vk_temporal_get_info)"""
    _fields_ = [("frames", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels_with_history", C.c_uint64)]


VK_DENOISE_FORM_AUTO, VK_DENOISE_FORM_PLAIN, VK_DENOISE_FORM_STAGED = range(3)      # vk_debug_denoise_form
VK_TREE_HANDED_OVER, VK_TREE_REBUILT_PROVEN, VK_TREE_REBUILT_EMPIRICAL, VK_TREE_REBUILT_FAST, VK_TREE_REBUILT_NEAR, VK_TREE_REBUILT_GRID = range(6)
VK_GATHER_NONE, VK_GATHER_PEER_COPY, VK_GATHER_RCCL = range(3)


class DebugLaunch(C.Structure):
    """vk_debug_launch of include/vecchio_amd_debug.h: one render_kernel launch of a scene's last frame"""
    _fields_ = [("role", C.c_uint32), ("features", C.c_uint32), ("lds_scene", C.c_uint32), ("minw", C.c_uint32), ("cost", C.c_uint32),
                ("grid_form", C.c_uint32), ("grid_size", C.c_uint32), ("block_size", C.c_uint32), ("shmem_bytes", C.c_uint32)]


(VK_LAUNCH_MAIN, VK_LAUNCH_DUAL_1024, VK_LAUNCH_DUAL_768, VK_LAUNCH_PROBE, VK_LAUNCH_REDO, VK_LAUNCH_FALLBACK) = range(6)


_host = None
_dev = None


def _build_locked(target, builder):
    """Build `target` (if missing or older than its sources) under an exclusive file lock, so that N ranks
    started together on a fresh checkout run ONE compile and nobody loads a half-written library: the
    builder writes to a temporary name and renames it into place."""
    import fcntl
    os.makedirs(LIB_DIR, exist_ok=True)
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            builder()
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    if not os.path.exists(target):
        raise RuntimeError(f"{target} was not built")


def load_host_lib():
    """libvecchio_host.so: scene builders / BVHNode::new / Camera::new (C++ mirror of scene.rs)."""
    global _host
    if _host is not None:
        return _host
    path = os.path.join(LIB_DIR, "libvecchio_host.so")
    from . import build
    if build.host_is_stale():
        _build_locked(path, build.build_host)   # a fresh or edited checkout: compile (g++), never substitute anything
    lib = C.CDLL(path)
    lib.vkh_scene_build.restype = C.c_void_p
    lib.vkh_scene_build.argtypes = [C.c_char_p, C.c_uint64]
    lib.vkh_scene_free.argtypes = [C.c_void_p]
    lib.vkh_scene_desc.restype = C.POINTER(SceneDesc)
    lib.vkh_scene_desc.argtypes = [C.c_void_p]
    lib.vkh_scene_next_camera.restype = C.c_int
    lib.vkh_scene_next_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
    lib.vkh_scene_defaults.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), F3]
    lib.vkh_camera_new.argtypes = [F3, F3, F3, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Camera)]
    lib.vkh_last_error.restype = C.c_char_p
    lib.vkh_write_ppm.restype = C.c_int
    lib.vkh_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.vkh_to_color.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.vkh_set_assets_dir.argtypes = [C.c_char_p]
    # the decoded copies of the reference's assets/*.png (data fixtures, tests/golden/make_assets.py)
    lib.vkh_set_assets_dir((os.environ.get("VECCHIO_ASSETS") or ASSETS_DIR).encode())
    _host = lib
    return lib


DEVICE_SYMBOLS = [
    "vk_abi_version", "vk_device_count", "vk_last_error", "vk_gather_backends", "vk_scene_create", "vk_scene_destroy",
    "vk_render", "vk_render_device", "vk_to_color_device", "vk_scene_get_info", "vk_scene_create_multi",
    "vk_scene_last_kernel_ms", "vk_scene_last_clamped_samples", "vk_scene_last_requeued_samples", "vk_scene_part_info",
    "vk_tile_slab_bytes", "vk_pack_tiles_device", "vk_unpack_tiles_device",
    "vk_progress_create", "vk_progress_step", "vk_progress_step_device", "vk_progress_reset", "vk_progress_stderr",
    "vk_progress_get_info", "vk_progress_destroy", "vk_progress_set_adaptive", "vk_progress_tile_samples",
    "vk_render_aov", "vk_render_aov_device",
    "vk_guide_default_params", "vk_render_guides", "vk_render_guides_device",
    "vk_trace_rays", "vk_trace_rays_device", "vk_trace_occluded", "vk_trace_occluded_device",
    "vk_trace_radiance", "vk_trace_irradiance", "vk_trace_probes", "vk_probe_eval", "vk_shade_hits",
    "vk_paths_create", "vk_paths_begin", "vk_paths_step", "vk_paths_read", "vk_paths_cull", "vk_paths_results", "vk_paths_get_info",
    "vk_paths_destroy", "vk_roulette_set", "vk_roulette_get",
    "vk_film_create", "vk_film_emit", "vk_film_deposit", "vk_film_resolve", "vk_film_reset", "vk_film_get_info", "vk_film_destroy",
    "vk_regen_begin", "vk_regen_step", "vk_regen_cull",
    "vk_adapt_enable", "vk_adapt_begin", "vk_adapt_close", "vk_adapt_resolve", "vk_adapt_stderr", "vk_adapt_tile_samples",
    "vk_splat_default_params", "vk_splat_create", "vk_splat_deposit", "vk_splat_resolve", "vk_splat_reset", "vk_splat_get_info",
    "vk_splat_destroy",
    "vk_robust_default_params", "vk_robust_create", "vk_robust_deposit", "vk_robust_resolve", "vk_robust_reset", "vk_robust_get_info",
    "vk_robust_destroy",
    "vk_lpe_create", "vk_lpe_step", "vk_lpe_tags", "vk_lpe_deposit", "vk_lpe_resolve", "vk_lpe_reset", "vk_lpe_get_info", "vk_lpe_destroy",
    "vk_tone_default_meter_params", "vk_tone_default_params", "vk_tone_create", "vk_tone_load", "vk_tone_load_device", "vk_tone_meter",
    "vk_tone_solve", "vk_tone_encode", "vk_tone_encode_device", "vk_tone_reset", "vk_tone_get_info", "vk_tone_destroy",
    "vk_nlm_default_params", "vk_nlm_create", "vk_nlm_load", "vk_nlm_load_device", "vk_nlm_filter", "vk_nlm_filter_device", "vk_nlm_reset",
    "vk_nlm_get_info", "vk_nlm_destroy",
    "vk_glare_default_params", "vk_glare_create", "vk_glare_apply", "vk_glare_apply_device", "vk_glare_get_info", "vk_glare_destroy",
    "vk_psf_default_params", "vk_psf_star", "vk_psf_create", "vk_psf_load", "vk_psf_load_device", "vk_psf_apply", "vk_psf_apply_device",
    "vk_psf_reset", "vk_psf_get_info", "vk_psf_destroy",
    "vk_upsample_default_params", "vk_upsample_create", "vk_upsample_load", "vk_upsample_load_device", "vk_upsample_apply",
    "vk_upsample_apply_device", "vk_upsample_reset", "vk_upsample_get_info", "vk_upsample_destroy",
    "vk_matte_default_params", "vk_render_mattes", "vk_matte_merge", "vk_matte_mask",
    "vk_denoise_default_params", "vk_denoise", "vk_denoise_device", "vk_progress_stderr_device",
    "vk_temporal_default_params", "vk_temporal_create", "vk_temporal_accumulate", "vk_temporal_accumulate_device", "vk_temporal_reset",
    "vk_temporal_get_info", "vk_temporal_destroy",
]


def device_lib_path():
    # VK_DEVICE_LIB: an alternate build of the same library (kernel experiments); never a different backend
    return os.environ.get("VK_DEVICE_LIB") or os.path.join(LIB_DIR, "libvecchio_amd.so")


def _bind(lib):
    """restype / argtypes of every entry point of include/vecchio_amd.h"""
    lib.vk_abi_version.restype = C.c_int
    lib.vk_gather_backends.restype = C.c_int
    lib.vk_device_count.restype = C.c_int
    lib.vk_last_error.restype = C.c_char_p
    lib.vk_scene_create.restype = C.c_int
    lib.vk_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
    lib.vk_scene_create_multi.restype = C.c_int
    lib.vk_scene_create_multi.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    lib.vk_scene_destroy.argtypes = [C.c_void_p]
    lib.vk_scene_last_kernel_ms.restype = C.c_int
    lib.vk_scene_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.vk_scene_last_clamped_samples.restype = C.c_int
    lib.vk_scene_last_clamped_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.vk_scene_last_requeued_samples.restype = C.c_int
    lib.vk_scene_last_requeued_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.vk_scene_part_info.restype = C.c_int
    lib.vk_scene_part_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(PartInfo)]
    lib.vk_render.restype = C.c_int
    lib.vk_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.POINTER(Stats)]
    lib.vk_render_device.restype = C.c_int
    lib.vk_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    lib.vk_to_color_device.restype = C.c_int
    lib.vk_to_color_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.vk_tile_slab_bytes.restype = C.c_size_t
    lib.vk_tile_slab_bytes.argtypes = [C.c_uint32] * 5
    for fn in (lib.vk_pack_tiles_device, lib.vk_unpack_tiles_device):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.vk_scene_get_info.restype = C.c_int
    lib.vk_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
    lib.vk_progress_create.restype = C.c_int
    lib.vk_progress_create.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_progress_step.restype = C.c_int
    lib.vk_progress_step.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(Stats)]
    lib.vk_progress_step_device.restype = C.c_int
    lib.vk_progress_step_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    lib.vk_progress_reset.restype = C.c_int
    lib.vk_progress_reset.argtypes = [C.c_void_p, C.POINTER(Camera)]
    lib.vk_progress_stderr.restype = C.c_int
    lib.vk_progress_stderr.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_progress_get_info.restype = C.c_int
    lib.vk_progress_get_info.argtypes = [C.c_void_p, C.POINTER(ProgressInfo)]
    lib.vk_progress_destroy.restype = None
    lib.vk_progress_destroy.argtypes = [C.c_void_p]
    lib.vk_progress_set_adaptive.restype = C.c_int
    lib.vk_progress_set_adaptive.argtypes = [C.c_void_p, C.POINTER(AdaptiveParams)]
    lib.vk_progress_tile_samples.restype = C.c_int
    lib.vk_progress_tile_samples.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AdaptiveInfo)]
    lib.vk_render_aov.restype = C.c_int
    lib.vk_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    lib.vk_render_aov_device.restype = C.c_int
    lib.vk_render_aov_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    lib.vk_guide_default_params.restype = C.c_int
    lib.vk_guide_default_params.argtypes = [C.POINTER(GuideParams)]
    lib.vk_render_guides.restype = C.c_int
    lib.vk_render_guides.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.POINTER(GuideParams)] + \
        [C.c_void_p] * 5 + [C.POINTER(Stats)]
    lib.vk_render_guides_device.restype = C.c_int
    lib.vk_render_guides_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.POINTER(GuideParams)] + \
        [C.c_void_p] * 6 + [C.POINTER(Stats)]
    lib.vk_trace_rays.restype = C.c_int
    lib.vk_trace_rays.argtypes = [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats)]
    lib.vk_trace_rays_device.restype = C.c_int
    lib.vk_trace_rays_device.argtypes = [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.POINTER(Stats)]
    lib.vk_trace_occluded.restype = C.c_int
    lib.vk_trace_occluded.argtypes = [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats)]
    lib.vk_trace_radiance.restype = C.c_int
    lib.vk_trace_radiance.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats)]
    lib.vk_trace_irradiance.restype = C.c_int
    lib.vk_trace_irradiance.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats)]
    lib.vk_trace_probes.restype = C.c_int
    lib.vk_trace_probes.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats)]
    lib.vk_shade_hits.restype = C.c_int
    lib.vk_shade_hits.argtypes = [C.c_void_p, C.POINTER(ShadeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.POINTER(Stats)]
    lib.vk_paths_create.restype = C.c_int
    lib.vk_paths_create.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.vk_paths_begin.restype = C.c_int
    lib.vk_paths_begin.argtypes = [C.c_void_p, C.POINTER(ShadeParams), C.c_void_p, C.c_void_p, C.c_uint64]
    lib.vk_paths_step.restype = C.c_int
    lib.vk_paths_step.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PathsStepInfo)]
    lib.vk_paths_read.restype = C.c_int
    lib.vk_paths_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_paths_cull.restype = C.c_int
    lib.vk_paths_cull.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_paths_results.restype = C.c_int
    lib.vk_paths_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_paths_get_info.restype = C.c_int
    lib.vk_paths_get_info.argtypes = [C.c_void_p, C.POINTER(PathsInfo)]
    lib.vk_paths_destroy.restype = None
    lib.vk_paths_destroy.argtypes = [C.c_void_p]
    lib.vk_roulette_set.restype = C.c_int
    lib.vk_roulette_set.argtypes = [C.c_void_p, C.POINTER(RouletteParams)]
    lib.vk_roulette_get.restype = C.c_int
    lib.vk_roulette_get.argtypes = [C.c_void_p, C.POINTER(RouletteParams), C.POINTER(C.c_int)]
    lib.vk_film_create.restype = C.c_int
    lib.vk_film_create.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(C.c_void_p)]
    lib.vk_film_emit.restype = C.c_int
    lib.vk_film_emit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FilmWindow)]
    lib.vk_film_deposit.restype = C.c_int
    lib.vk_film_deposit.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_film_resolve.restype = C.c_int
    lib.vk_film_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vk_film_reset.restype = C.c_int
    lib.vk_film_reset.argtypes = [C.c_void_p, C.POINTER(Camera)]
    lib.vk_film_get_info.restype = C.c_int
    lib.vk_film_get_info.argtypes = [C.c_void_p, C.POINTER(FilmInfo)]
    lib.vk_film_destroy.restype = None
    lib.vk_film_destroy.argtypes = [C.c_void_p]
    lib.vk_regen_begin.restype = C.c_int
    lib.vk_regen_begin.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(FilmWindow)]
    lib.vk_regen_step.restype = C.c_int
    lib.vk_regen_step.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RegenInfo)]
    lib.vk_regen_cull.restype = C.c_int
    lib.vk_regen_cull.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_adapt_enable.restype = C.c_int
    lib.vk_adapt_enable.argtypes = [C.c_void_p, C.POINTER(AdaptiveParams)]
    lib.vk_adapt_begin.restype = C.c_int
    lib.vk_adapt_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.vk_adapt_close.restype = C.c_int
    lib.vk_adapt_close.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(AdaptInfo)]
    lib.vk_adapt_resolve.restype = C.c_int
    lib.vk_adapt_resolve.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_adapt_stderr.restype = C.c_int
    lib.vk_adapt_stderr.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_adapt_tile_samples.restype = C.c_int
    lib.vk_adapt_tile_samples.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AdaptiveInfo)]
    lib.vk_splat_default_params.restype = C.c_int
    lib.vk_splat_default_params.argtypes = [C.POINTER(SplatParams)]
    lib.vk_splat_create.restype = C.c_int
    lib.vk_splat_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SplatParams), C.POINTER(C.c_void_p)]
    lib.vk_splat_deposit.restype = C.c_int
    lib.vk_splat_deposit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_splat_resolve.restype = C.c_int
    lib.vk_splat_resolve.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_splat_reset.restype = C.c_int
    lib.vk_splat_reset.argtypes = [C.c_void_p]
    lib.vk_splat_get_info.restype = C.c_int
    lib.vk_splat_get_info.argtypes = [C.c_void_p, C.POINTER(SplatInfo)]
    lib.vk_splat_destroy.restype = None
    lib.vk_splat_destroy.argtypes = [C.c_void_p]
    lib.vk_robust_default_params.restype = C.c_int
    lib.vk_robust_default_params.argtypes = [C.POINTER(RobustParams)]
    lib.vk_robust_create.restype = C.c_int
    lib.vk_robust_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RobustParams), C.POINTER(C.c_void_p)]
    lib.vk_robust_deposit.restype = C.c_int
    lib.vk_robust_deposit.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_robust_resolve.restype = C.c_int
    lib.vk_robust_resolve.argtypes = [C.c_void_p, C.POINTER(RobustParams), C.c_void_p, C.c_void_p]
    lib.vk_robust_reset.restype = C.c_int
    lib.vk_robust_reset.argtypes = [C.c_void_p]
    lib.vk_robust_get_info.restype = C.c_int
    lib.vk_robust_get_info.argtypes = [C.c_void_p, C.POINTER(RobustInfo)]
    lib.vk_robust_destroy.restype = None
    lib.vk_robust_destroy.argtypes = [C.c_void_p]
    lib.vk_lpe_create.restype = C.c_int
    lib.vk_lpe_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(LpeParams), C.POINTER(C.c_void_p)]
    lib.vk_lpe_step.restype = C.c_int
    lib.vk_lpe_step.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(PathsStepInfo)]
    lib.vk_lpe_tags.restype = C.c_int
    lib.vk_lpe_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_lpe_deposit.restype = C.c_int
    lib.vk_lpe_deposit.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_lpe_resolve.restype = C.c_int
    lib.vk_lpe_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.vk_lpe_reset.restype = C.c_int
    lib.vk_lpe_reset.argtypes = [C.c_void_p]
    lib.vk_lpe_get_info.restype = C.c_int
    lib.vk_lpe_get_info.argtypes = [C.c_void_p, C.POINTER(LpeInfo)]
    lib.vk_lpe_destroy.restype = None
    lib.vk_lpe_destroy.argtypes = [C.c_void_p]
    lib.vk_tone_default_meter_params.restype = C.c_int
    lib.vk_tone_default_meter_params.argtypes = [C.POINTER(ToneMeterParams)]
    lib.vk_tone_default_params.restype = C.c_int
    lib.vk_tone_default_params.argtypes = [C.POINTER(ToneParams)]
    lib.vk_tone_create.restype = C.c_int
    lib.vk_tone_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_tone_load.restype = C.c_int
    lib.vk_tone_load.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_tone_load_device.restype = C.c_int
    lib.vk_tone_load_device.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_tone_meter.restype = C.c_int
    lib.vk_tone_meter.argtypes = [C.c_void_p, C.POINTER(ToneMeterParams), C.POINTER(ToneMeterInfo)]
    lib.vk_tone_solve.restype = C.c_int
    lib.vk_tone_solve.argtypes = [C.c_void_p, C.POINTER(ToneMeterParams), C.POINTER(C.c_double), C.POINTER(ToneMeterInfo)]
    lib.vk_tone_encode.restype = C.c_int
    lib.vk_tone_encode.argtypes = [C.c_void_p, C.POINTER(ToneParams), C.c_void_p]
    lib.vk_tone_encode_device.restype = C.c_int
    lib.vk_tone_encode_device.argtypes = [C.c_void_p, C.POINTER(ToneParams), C.c_void_p]
    lib.vk_tone_reset.restype = C.c_int
    lib.vk_tone_reset.argtypes = [C.c_void_p]
    lib.vk_tone_get_info.restype = C.c_int
    lib.vk_tone_get_info.argtypes = [C.c_void_p, C.POINTER(ToneInfo)]
    lib.vk_tone_destroy.restype = None
    lib.vk_tone_destroy.argtypes = [C.c_void_p]
    lib.vk_nlm_default_params.restype = C.c_int
    lib.vk_nlm_default_params.argtypes = [C.POINTER(NlmParams)]
    lib.vk_nlm_create.restype = C.c_int
    lib.vk_nlm_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_nlm_load.restype = C.c_int
    lib.vk_nlm_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_nlm_load_device.restype = C.c_int
    lib.vk_nlm_load_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_nlm_filter.restype = C.c_int
    lib.vk_nlm_filter.argtypes = [C.c_void_p, C.POINTER(NlmParams), C.c_void_p, C.c_void_p]
    lib.vk_nlm_filter_device.restype = C.c_int
    lib.vk_nlm_filter_device.argtypes = [C.c_void_p, C.POINTER(NlmParams), C.c_void_p, C.c_void_p]
    lib.vk_nlm_reset.restype = C.c_int
    lib.vk_nlm_reset.argtypes = [C.c_void_p]
    lib.vk_nlm_get_info.restype = C.c_int
    lib.vk_nlm_get_info.argtypes = [C.c_void_p, C.POINTER(NlmInfo)]
    lib.vk_nlm_destroy.restype = None
    lib.vk_nlm_destroy.argtypes = [C.c_void_p]
    lib.vk_glare_default_params.restype = C.c_int
    lib.vk_glare_default_params.argtypes = [C.POINTER(GlareParams)]
    lib.vk_glare_create.restype = C.c_int
    lib.vk_glare_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_glare_apply.restype = C.c_int
    lib.vk_glare_apply.argtypes = [C.c_void_p, C.POINTER(GlareParams), C.c_void_p, C.c_void_p]
    lib.vk_glare_apply_device.restype = C.c_int
    lib.vk_glare_apply_device.argtypes = [C.c_void_p, C.POINTER(GlareParams), C.c_void_p, C.c_void_p]
    lib.vk_glare_get_info.restype = C.c_int
    lib.vk_glare_get_info.argtypes = [C.c_void_p, C.POINTER(GlareInfo)]
    lib.vk_glare_destroy.restype = None
    lib.vk_glare_destroy.argtypes = [C.c_void_p]
    lib.vk_psf_default_params.restype = C.c_int
    lib.vk_psf_default_params.argtypes = [C.POINTER(PsfParams)]
    lib.vk_psf_star.restype = C.c_int
    lib.vk_psf_star.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.vk_psf_create.restype = C.c_int
    lib.vk_psf_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_psf_load.restype = C.c_int
    lib.vk_psf_load.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vk_psf_load_device.restype = C.c_int
    lib.vk_psf_load_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vk_psf_apply.restype = C.c_int
    lib.vk_psf_apply.argtypes = [C.c_void_p, C.POINTER(PsfParams), C.c_void_p, C.c_void_p]
    lib.vk_psf_apply_device.restype = C.c_int
    lib.vk_psf_apply_device.argtypes = [C.c_void_p, C.POINTER(PsfParams), C.c_void_p, C.c_void_p]
    lib.vk_psf_reset.restype = C.c_int
    lib.vk_psf_reset.argtypes = [C.c_void_p]
    lib.vk_psf_get_info.restype = C.c_int
    lib.vk_psf_get_info.argtypes = [C.c_void_p, C.POINTER(PsfInfo)]
    lib.vk_psf_destroy.restype = None
    lib.vk_psf_destroy.argtypes = [C.c_void_p]
    lib.vk_upsample_default_params.restype = C.c_int
    lib.vk_upsample_default_params.argtypes = [C.POINTER(UpsampleParams)]
    lib.vk_upsample_create.restype = C.c_int
    lib.vk_upsample_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.vk_upsample_load.restype = C.c_int
    lib.vk_upsample_load.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.vk_upsample_load_device.restype = C.c_int
    lib.vk_upsample_load_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.vk_upsample_apply.restype = C.c_int
    lib.vk_upsample_apply.argtypes = [C.c_void_p, C.POINTER(UpsampleParams)] + [C.c_void_p] * 5
    lib.vk_upsample_apply_device.restype = C.c_int
    lib.vk_upsample_apply_device.argtypes = [C.c_void_p, C.POINTER(UpsampleParams)] + [C.c_void_p] * 5
    lib.vk_upsample_reset.restype = C.c_int
    lib.vk_upsample_reset.argtypes = [C.c_void_p]
    lib.vk_upsample_get_info.restype = C.c_int
    lib.vk_upsample_get_info.argtypes = [C.c_void_p, C.POINTER(UpsampleInfo)]
    lib.vk_upsample_destroy.restype = None
    lib.vk_upsample_destroy.argtypes = [C.c_void_p]
    lib.vk_matte_default_params.restype = C.c_int
    lib.vk_matte_default_params.argtypes = [C.POINTER(MatteParams)]
    lib.vk_render_mattes.restype = C.c_int
    lib.vk_render_mattes.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.POINTER(MatteParams),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    lib.vk_matte_merge.restype = C.c_int
    lib.vk_matte_merge.argtypes = [C.c_uint32, C.c_uint64] + [C.c_void_p] * 6
    lib.vk_matte_mask.restype = C.c_int
    lib.vk_matte_mask.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vk_probe_eval.restype = C.c_int
    lib.vk_probe_eval.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float)]
    lib.vk_trace_occluded_device.restype = C.c_int
    lib.vk_trace_occluded_device.argtypes = [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.POINTER(Stats)]
    lib.vk_denoise_default_params.restype = C.c_int
    lib.vk_denoise_default_params.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams)]
    lib.vk_denoise.restype = C.c_int
    lib.vk_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)] + [C.c_void_p] * 6 + [C.POINTER(Stats)]
    lib.vk_denoise_device.restype = C.c_int
    lib.vk_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)] + [C.c_void_p] * 7
    lib.vk_progress_stderr_device.restype = C.c_int
    lib.vk_progress_stderr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_temporal_default_params.restype = C.c_int
    lib.vk_temporal_default_params.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)]
    lib.vk_temporal_create.restype = C.c_int
    lib.vk_temporal_create.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(C.c_void_p)]
    lib.vk_temporal_accumulate.restype = C.c_int
    lib.vk_temporal_accumulate.argtypes = [C.c_void_p, C.POINTER(Camera)] + [C.c_void_p] * 8 + [C.POINTER(Stats)]
    lib.vk_temporal_accumulate_device.restype = C.c_int
    lib.vk_temporal_accumulate_device.argtypes = [C.c_void_p, C.POINTER(Camera)] + [C.c_void_p] * 9
    lib.vk_temporal_reset.restype = C.c_int
    lib.vk_temporal_reset.argtypes = [C.c_void_p]
    lib.vk_temporal_get_info.restype = C.c_int
    lib.vk_temporal_get_info.argtypes = [C.c_void_p, C.POINTER(TemporalInfo)]
    lib.vk_temporal_destroy.restype = None
    lib.vk_temporal_destroy.argtypes = [C.c_void_p]
    lib.vk_debug_denoise_form.restype = C.c_int
    lib.vk_debug_denoise_form.argtypes = [C.c_void_p, C.c_int]
    lib.vk_debug_denoise_last_ms.restype = C.c_int
    lib.vk_debug_denoise_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 9)]
    # the test hooks of include/vecchio_amd_debug.h that the product library carries too
    lib.vk_debug_last_launches.restype = C.c_int
    lib.vk_debug_last_launches.argtypes = [C.c_void_p, C.POINTER(DebugLaunch), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.vk_debug_progress_moments.restype = C.c_int
    lib.vk_debug_progress_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_debug_trace_radiance_samples.restype = C.c_int
    lib.vk_debug_trace_radiance_samples.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                    C.POINTER(Stats)]
    lib.vk_debug_trace_irradiance_samples.restype = C.c_int
    lib.vk_debug_trace_irradiance_samples.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                      C.POINTER(Stats)]
    lib.vk_debug_trace_probe_samples.restype = C.c_int
    lib.vk_debug_trace_probe_samples.argtypes = [C.c_void_p, C.POINTER(RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                 C.POINTER(Stats)]
    lib.vk_debug_compact_paths.restype = C.c_int
    lib.vk_debug_compact_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5 + \
        [C.POINTER(C.c_uint64 * 5)]
    lib.vk_debug_compact_roulette.restype = C.c_int
    lib.vk_debug_compact_roulette.argtypes = [C.c_void_p, C.POINTER(RouletteParams), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + \
        [C.c_void_p] * 5 + [C.POINTER(C.c_uint64 * 5)]
    lib.vk_debug_paths_last_ms.restype = C.c_int
    lib.vk_debug_paths_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 3)]
    lib.vk_debug_film_sums.restype = C.c_int
    lib.vk_debug_film_sums.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_debug_film_last_ms.restype = C.c_int
    lib.vk_debug_film_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 3)]
    lib.vk_debug_film_deposit_form.restype = C.c_int
    lib.vk_debug_film_deposit_form.argtypes = [C.c_void_p, C.c_int]
    lib.vk_debug_regen_last_ms.restype = C.c_int
    lib.vk_debug_regen_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 4)]
    lib.vk_debug_adapt_moments.restype = C.c_int
    lib.vk_debug_adapt_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_debug_adapt_set_tiles.restype = C.c_int
    lib.vk_debug_adapt_set_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_debug_adapt_sequence.restype = C.c_int
    lib.vk_debug_adapt_sequence.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.vk_debug_splat_sums.restype = C.c_int
    lib.vk_debug_splat_sums.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_debug_splat_form.restype = C.c_int
    lib.vk_debug_splat_form.argtypes = [C.c_void_p, C.c_uint32]
    lib.vk_debug_splat_last_ms.restype = C.c_int
    lib.vk_debug_splat_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 2)]
    lib.vk_debug_robust_sums.restype = C.c_int
    lib.vk_debug_robust_sums.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_debug_robust_last_ms.restype = C.c_int
    lib.vk_debug_robust_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 2)]
    lib.vk_debug_lpe_sums.restype = C.c_int
    lib.vk_debug_lpe_sums.argtypes = [C.c_void_p, C.c_void_p]
    lib.vk_debug_lpe_set_tags.restype = C.c_int
    lib.vk_debug_lpe_set_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_debug_lpe_last_ms.restype = C.c_int
    lib.vk_debug_lpe_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 3)]
    lib.vk_debug_tone_histogram.restype = C.c_int
    lib.vk_debug_tone_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vk_debug_tone_table.restype = C.c_int
    lib.vk_debug_tone_table.argtypes = [C.c_uint32, C.c_void_p]
    lib.vk_debug_tone_set_form.restype = C.c_int
    lib.vk_debug_tone_set_form.argtypes = [C.c_void_p, C.c_uint32]
    lib.vk_debug_tone_last_ms.restype = C.c_int
    lib.vk_debug_tone_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 2)]
    lib.vk_debug_nlm_set_form.restype = C.c_int
    lib.vk_debug_nlm_set_form.argtypes = [C.c_void_p, C.c_uint32]
    lib.vk_debug_nlm_last_ms.restype = C.c_int
    lib.vk_debug_nlm_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 2)]
    lib.vk_debug_glare_set_form.restype = C.c_int
    lib.vk_debug_glare_set_form.argtypes = [C.c_void_p, C.c_uint32]
    lib.vk_debug_glare_last_ms.restype = C.c_int
    lib.vk_debug_glare_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.vk_psf_debug_twiddles.restype = C.c_int
    lib.vk_psf_debug_twiddles.argtypes = [C.c_uint32, C.c_void_p]
    lib.vk_psf_debug_last_pass_ms.restype = C.c_int
    lib.vk_psf_debug_last_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 4)]
    lib.vk_psf_debug_fft2.restype = C.c_int
    lib.vk_psf_debug_fft2.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.vk_debug_upsample_set_form.restype = C.c_int
    lib.vk_debug_upsample_set_form.argtypes = [C.c_void_p, C.c_uint32]
    lib.vk_debug_upsample_last_ms.restype = C.c_int
    lib.vk_debug_upsample_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.vk_debug_matte_samples.restype = C.c_int
    lib.vk_debug_matte_samples.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.c_uint32, C.c_void_p]
    lib.vk_debug_trace_occluded_device.restype = C.c_int
    lib.vk_debug_trace_occluded_device.argtypes = [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_uint32, C.c_uint32]


_dbg = None


def load_debug_lib():
    """libvecchio_amd_debug.so: the same sources built with -DVK_DEBUG_LIB (instrumented kernel builds, device arithmetic probe:
    include/vecchio_amd_debug.h).  TESTS AND DIAGNOSTICS ONLY.  A vk_scene belongs to the library that created it:
    DeviceScene(desc, lib=load_debug_lib())."""
    global _dbg
    if _dbg is not None:
        return _dbg
    path = os.path.join(LIB_DIR, "libvecchio_amd_debug.so")
    from . import build
    if build.debug_is_stale():
        _build_locked(path, build.build_device_debug)
    lib = C.CDLL(path)
    _bind(lib)
    lib.vk_debug_phase_stats.restype = C.c_int
    lib.vk_debug_phase_stats.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(C.c_uint64 * 24)]
    lib.vk_debug_math.restype = C.c_int
    lib.vk_debug_math.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.vk_debug_live_objects.restype = C.c_int
    lib.vk_debug_live_objects.argtypes = [C.POINTER(C.c_uint64 * 4)]
    _dbg = lib
    return lib


def last_launches(lib, handle):
    """the render_kernel launches of the scene's last frame (vk_debug_last_launches), as a list of DebugLaunch"""
    n = C.c_uint32()
    assert lib.vk_debug_last_launches(handle, None, 0, C.byref(n)) == VK_OK, lib.vk_last_error().decode()
    out = (DebugLaunch * max(1, n.value))()
    assert lib.vk_debug_last_launches(handle, out, n.value, C.byref(n)) == VK_OK, lib.vk_last_error().decode()
    return list(out[:n.value])


def load_device_lib():
    """libvecchio_amd.so: the HIP product behind include/vecchio_amd.h.  Fails loudly if absent."""
    global _dev
    if _dev is not None:
        return _dev
    path = device_lib_path()
    from . import build
    if not os.environ.get("VK_DEVICE_LIB") and build.device_is_stale():
        try:                        # a fresh or edited checkout: compile with hipcc; there is no CPU fallback to use instead
            _build_locked(path, build.build_device)
        except Exception as e:
            raise RuntimeError(f"{path} missing or stale and hipcc could not build it ({e}); the HIP extension is required "
                               "(no CPU fallback exists)") from e
    lib = C.CDLL(path)
    _bind(lib)
    _dev = lib
    return lib
