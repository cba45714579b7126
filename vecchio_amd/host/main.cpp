// main.cpp — harness playing the role of the reference's main() (main.rs:155-221): pick a
// scene, build the BVH, upload once, then per Camera of cam_iter: render through the C ABI
// (the call that replaces main.rs:181-198), write output_%04d.ppm, print the frame time.
// The reference hard-codes scene/width/spp/depth (main.rs:28-29,159-167,171); here they are
// arguments:   vecchio_cli <scene> [width=900] [spp=1000] [max_depth=100] [frames=1] [seed=1] [steps=1] [aov_spp=0] [denoise=0] [temporal=0] [guide_bounces=0] [display=0] [glare=0] [scale=0] [psf=0]
// steps > 1: each frame is rendered progressively (vk_progress_*) in `steps` equal sample windows; after each window the running image
// is written to output_%04d_step%02d.ppm and the samples done and the image's mean relative standard error are printed.  The final
// output_%04d.ppm is byte-identical to the one of steps = 1.
// aov_spp > 0: each frame also writes its f32 image as output_%04d.pfm and the first-hit buffers of samples 0 .. aov_spp-1
// (vk_render_aov) as output_%04d_albedo.pfm, _normal.pfm (PF, 3 channels), _depth.pfm and _coverage.pfm (Pf, 1 channel): little-endian
// (scale -1), rows bottom to top as PFM stores them — the library's y-up buffers as they are.  What a denoiser takes; the .ppm is unchanged.
// denoise = 1 (needs steps >= 2 and aov_spp > 0): each frame is also denoised on the device (vk_denoise with the library's default parameters)
// from its final mean, its final standard error and the first-hit buffers, and written as output_%04d_denoised.ppm and .pfm.
// temporal = 1 (needs steps >= 2 and aov_spp > 0): the frames share one temporal accumulator (vk_temporal_* with the library's default
// parameters); frame i is rendered with seed + 1 + i, so that the frames are independent, reprojected into the history and written as
// output_%04d_temporal.ppm and .pfm; with denoise = 1 the denoised files are filtered from the accumulated colour and standard error.
// With temporal = 0 the seed does not change and every file is what it was.
// guide_bounces > 0 (needs aov_spp > 0; at most 8): the specular guides of the same samples (vk_render_guides, max_bounces = guide_bounces,
// the other parameters the library's defaults) are written as output_%04d_guide_albedo.pfm, _guide_normal.pfm, _guide_depth.pfm and
// _guide_bounces.pfm, and the temporal and denoise steps take their albedo, normal and depth from them instead of from the first-hit
// buffers.  0 or absent: no such call is made and every file is what it was.
// display = 1, 2 or 3: each frame's last float image — the denoised one, else the temporally accumulated one, else the plain frame — also
// goes through the display transform (vk_tone_*): metered with the library's default parameters (over an animation, frames > 1, with
// blend 0.25, so that the exposure follows the frames smoothly), encoded with the Reinhard (1), Hable (2) or ACES (3) curve, the metered
// exposure and the sRGB transfer, and written as output_%04d_display.ppm.  display = 0 or absent: every file is what it was.
// glare = 1 .. 100: that frame — display's, whether or not display is on — first goes through the glare stage (vk_glare_*) with strength
// glare / 100 and the library's other default parameters; the result is written as output_%04d_glare.pfm and is what display encodes.
// glare = 0 or absent: no such call is made and every file is what it was.
// psf = 1 .. 64: the number of streaks of an aperture star.  That frame — after glare, if glare is on — goes through the point-spread
// stage (vk_psf_*) with the 65 x 65 kernel of vk_psf_star(65, psf, 0, 8, 0.1) and the library's default parameters; the result is written
// as output_%04d_psf.pfm and is what display encodes.  psf = 0 or absent: no such call is made and every file is what it was.
// scale = 1 .. 99 (needs aov_spp > 0): render scale in percent.  The paths — and with steps > 1 their standard error — are traced at
// width * scale / 100 (output_%04d.ppm, its steps and output_%04d.pfm are that low frame), the first-hit buffers are rendered at that
// size too (output_%04d_lo_albedo.pfm, _lo_normal.pfm, _lo_depth.pfm) and at full size, and guided upsampling (vk_upsample_* with the
// library's default parameters) brings the frame and its standard error to full size: output_%04d_upsampled.ppm and .pfm.  The temporal,
// denoise, glare and display steps then run on that frame at full size.  scale = 0, 100 or absent: no such call is made and every file
// is what it was.
// Texture images are read from ./assets (as in the reference) or $VECCHIO_ASSETS: <name>.ppm.gz, see host_api.h.
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_api.h"

// PFM: "PF" (3 channels) or "Pf" (1), width height, scale -1 = little-endian floats, rows bottom to top
static bool write_pfm(const char *fn, const float *data, uint32_t width, uint32_t height, int channels) {
    FILE *f = fopen(fn, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", fn); return false; }
    fprintf(f, "%s\n%u %u\n-1\n", channels == 3 ? "PF" : "Pf", width, height);
    const size_t n = (size_t)width * height * channels;
    const bool ok = fwrite(data, sizeof(float), n, f) == n;      // (gfx950 hosts are little-endian)
    return fclose(f) == 0 && ok;
}

// the display transform's 8-bit codes (row 0 the top) in vkh_write_ppm's P3 layout
static bool write_ppm_codes(const char *fn, const uint8_t *rgb8, uint32_t width, uint32_t height) {
    FILE *f = fopen(fn, "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", fn); return false; }
    fprintf(f, "P3\n%u %u\n255\n", width, height);
    for (size_t i = 0; i < (size_t)width * height; i++) fprintf(f, "%u %u %u\n", rgb8[i * 3], rgb8[i * 3 + 1], rgb8[i * 3 + 2]);
    return fclose(f) == 0;
}

template <class T>
static T sym(void *h, const char *name) {
    void *p = dlsym(h, name);
    if (!p) { fprintf(stderr, "missing symbol %s\n", name); exit(2); }
    return reinterpret_cast<T>(p);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <balls_demo|random_spheres_demo|random_spheres_iow|perlin_demo|bowser_demo|cornell_box|final_scene|"
                        "final_scene_nextweek|stress_spheres:N> [width] [spp] [max_depth] [frames] [seed] [steps] [aov_spp] [denoise] [temporal] [guide_bounces] [display] [glare] [scale] [psf]\n", argv[0]);
        return 2;
    }
    const char *name = argv[1];
    uint32_t width = argc > 2 ? (uint32_t)atoi(argv[2]) : 900;       // main.rs:171
    uint32_t spp = argc > 3 ? (uint32_t)atoi(argv[3]) : 1000;        // main.rs:28
    uint32_t depth = argc > 4 ? (uint32_t)atoi(argv[4]) : 100;       // main.rs:29
    int frames = argc > 5 ? atoi(argv[5]) : 1;
    uint64_t seed = argc > 6 ? strtoull(argv[6], nullptr, 10) : 1;
    uint32_t steps = argc > 7 ? (uint32_t)atoi(argv[7]) : 1;
    uint32_t aov_spp = argc > 8 ? (uint32_t)atoi(argv[8]) : 0;
    const bool denoise = argc > 9 && atoi(argv[9]) != 0;
    const bool temporal = argc > 10 && atoi(argv[10]) != 0;
    const uint32_t guide_bounces = argc > 11 ? (uint32_t)atoi(argv[11]) : 0;
    const uint32_t display = argc > 12 ? (uint32_t)atoi(argv[12]) : 0;
    if (display > 3) {
        fprintf(stderr, "display is 0 (off), 1 (Reinhard), 2 (Hable) or 3 (ACES)\n");
        return 2;
    }
    const uint32_t glare_pct = argc > 13 ? (uint32_t)atoi(argv[13]) : 0;
    if (glare_pct > 100) {
        fprintf(stderr, "glare is the strength in percent: 0 (off) to 100\n");
        return 2;
    }
    const uint32_t scale_pct = argc > 14 ? (uint32_t)atoi(argv[14]) : 0;
    if (scale_pct > 100) {
        fprintf(stderr, "scale is the render scale in percent: 1 to 99; 0 or 100 is off\n");
        return 2;
    }
    const bool scaled = scale_pct != 0 && scale_pct != 100;
    const uint32_t psf_streaks = argc > 15 ? (uint32_t)atoi(argv[15]) : 0;
    if (psf_streaks > 64) {
        fprintf(stderr, "psf is the number of streaks of the aperture star: 1 to 64; 0 is off\n");
        return 1;
    }
    constexpr uint32_t PSF_K = 65;
    if (scaled && aov_spp == 0) {
        fprintf(stderr, "scale needs the first-hit buffers at both sizes: aov_spp > 0\n");
        return 2;
    }
    if (steps < 1) steps = 1;
    if (steps > spp) steps = spp;                                     // every window holds at least one sample
    if (denoise && (steps < 2 || aov_spp == 0)) {
        fprintf(stderr, "denoise = 1 needs the standard error and the first-hit buffers: steps >= 2 and aov_spp > 0\n");
        return 2;
    }
    if (temporal && (steps < 2 || aov_spp == 0)) {
        fprintf(stderr, "temporal = 1 needs the standard error and the first-hit buffers: steps >= 2 and aov_spp > 0\n");
        return 2;
    }
    if (guide_bounces > 0 && aov_spp == 0) {
        fprintf(stderr, "guide_bounces > 0 renders the guides of the first-hit samples: aov_spp > 0\n");
        return 2;
    }

    std::string dir = argv[0];
    size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? "." : dir.substr(0, slash);
    void *h = dlopen((dir + "/libvecchio_amd.so").c_str(), RTLD_NOW);
    if (!h) { fprintf(stderr, "cannot load libvecchio_amd.so: %s\n", dlerror()); return 2; }
    auto p_create = sym<int (*)(const vk_scene_desc *, int, vk_scene **)>(h, "vk_scene_create");
    auto p_render = sym<int (*)(vk_scene *, const vk_camera *, const vk_render_params *, float *, vk_stats *)>(h, "vk_render");
    auto p_destroy = sym<void (*)(vk_scene *)>(h, "vk_scene_destroy");
    auto p_err = sym<const char *(*)()>(h, "vk_last_error");
    auto p_pcreate = sym<int (*)(vk_scene *, const vk_camera *, const vk_render_params *, uint32_t, vk_progress **)>(h, "vk_progress_create");
    auto p_pstep = sym<int (*)(vk_progress *, uint32_t, void *, vk_stats *)>(h, "vk_progress_step");
    auto p_pstderr = sym<int (*)(vk_progress *, float *)>(h, "vk_progress_stderr");
    auto p_pdestroy = sym<void (*)(vk_progress *)>(h, "vk_progress_destroy");
    auto p_aov = sym<int (*)(vk_scene *, const vk_camera *, const vk_render_params *, uint32_t, float *, float *, float *, float *, vk_stats *)>(
        h, "vk_render_aov");
    auto p_gp_defaults = sym<int (*)(vk_guide_params *)>(h, "vk_guide_default_params");
    auto p_guides = sym<int (*)(vk_scene *, const vk_camera *, const vk_render_params *, uint32_t, const vk_guide_params *, float *, float *,
                                float *, float *, float *, vk_stats *)>(h, "vk_render_guides");
    auto p_dn_defaults = sym<int (*)(uint32_t, uint32_t, vk_denoise_params *)>(h, "vk_denoise_default_params");
    auto p_denoise = sym<int (*)(vk_scene *, const vk_denoise_params *, const float *, const float *, const float *, const float *, const float *,
                                 float *, vk_stats *)>(h, "vk_denoise");
    auto p_tp_defaults = sym<int (*)(uint32_t, uint32_t, vk_temporal_params *)>(h, "vk_temporal_default_params");
    auto p_tcreate = sym<int (*)(vk_scene *, const vk_temporal_params *, vk_temporal **)>(h, "vk_temporal_create");
    auto p_taccum = sym<int (*)(vk_temporal *, const vk_camera *, const float *, const float *, const float *, const float *, const float *,
                                float *, float *, float *, vk_stats *)>(h, "vk_temporal_accumulate");
    auto p_tinfo = sym<int (*)(vk_temporal *, vk_temporal_info *)>(h, "vk_temporal_get_info");
    auto p_tdestroy = sym<void (*)(vk_temporal *)>(h, "vk_temporal_destroy");
    auto p_tone_mdefaults = sym<int (*)(vk_tone_meter_params *)>(h, "vk_tone_default_meter_params");
    auto p_tone_defaults = sym<int (*)(vk_tone_params *)>(h, "vk_tone_default_params");
    auto p_tone_create = sym<int (*)(vk_scene *, uint32_t, uint32_t, vk_tone **)>(h, "vk_tone_create");
    auto p_tone_load = sym<int (*)(vk_tone *, const float *)>(h, "vk_tone_load");
    auto p_tone_meter = sym<int (*)(vk_tone *, const vk_tone_meter_params *, vk_tone_meter_info *)>(h, "vk_tone_meter");
    auto p_tone_encode = sym<int (*)(vk_tone *, const vk_tone_params *, uint8_t *)>(h, "vk_tone_encode");
    auto p_tone_destroy = sym<void (*)(vk_tone *)>(h, "vk_tone_destroy");
    auto p_glare_defaults = sym<int (*)(vk_glare_params *)>(h, "vk_glare_default_params");
    auto p_glare_create = sym<int (*)(vk_scene *, uint32_t, uint32_t, vk_glare **)>(h, "vk_glare_create");
    auto p_glare_apply = sym<int (*)(vk_glare *, const vk_glare_params *, const float *, float *)>(h, "vk_glare_apply");
    auto p_glare_destroy = sym<void (*)(vk_glare *)>(h, "vk_glare_destroy");
    auto p_psf_defaults = sym<int (*)(vk_psf_params *)>(h, "vk_psf_default_params");
    auto p_psf_star = sym<int (*)(uint32_t, uint32_t, float, float, float, float *)>(h, "vk_psf_star");
    auto p_psf_create = sym<int (*)(vk_scene *, uint32_t, uint32_t, uint32_t, vk_psf **)>(h, "vk_psf_create");
    auto p_psf_load = sym<int (*)(vk_psf *, uint32_t, const float *)>(h, "vk_psf_load");
    auto p_psf_apply = sym<int (*)(vk_psf *, const vk_psf_params *, const float *, float *)>(h, "vk_psf_apply");
    auto p_psf_destroy = sym<void (*)(vk_psf *)>(h, "vk_psf_destroy");
    auto p_up_defaults = sym<int (*)(vk_upsample_params *)>(h, "vk_upsample_default_params");
    auto p_up_create = sym<int (*)(vk_scene *, uint32_t, uint32_t, uint32_t, uint32_t, vk_upsample **)>(h, "vk_upsample_create");
    auto p_up_load = sym<int (*)(vk_upsample *, const float *, const float *, const float *, const float *, const float *)>(h, "vk_upsample_load");
    auto p_up_apply = sym<int (*)(vk_upsample *, const vk_upsample_params *, const float *, const float *, const float *, float *, float *)>(
        h, "vk_upsample_apply");
    auto p_up_info = sym<int (*)(vk_upsample *, vk_upsample_info *)>(h, "vk_upsample_get_info");
    auto p_up_destroy = sym<void (*)(vk_upsample *)>(h, "vk_upsample_destroy");

    fprintf(stderr, "Generating scene...\n");                        // main.rs:157
    vkh_scene *hs = vkh_scene_build(name, seed);
    if (!hs) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
    float aspect; uint32_t integ, bg; float bgc[3];
    vkh_scene_defaults(hs, &aspect, &integ, &bg, bgc);
    uint32_t height = (uint32_t)((float)width / aspect);              // main.rs:172
    vk_scene *scene = nullptr;
    if (p_create(vkh_scene_desc(hs), 0, &scene) != VK_OK) { fprintf(stderr, "vk_scene_create: %s\n", p_err()); return 1; }

    std::vector<float> pixels((size_t)width * height * 3, 0.0f);     // main.rs:173
    // the size the paths are traced at, and the frame they land in: the full one, or the low one of a render scale
    const uint32_t lw = scaled ? (uint32_t)((uint64_t)width * scale_pct / 100u) : width;
    const uint32_t lh = scaled ? (uint32_t)((float)lw / aspect) : height;
    std::vector<float> low(scaled ? (size_t)lw * lh * 3 : 0, 0.0f);
    float *const traced = scaled ? low.data() : pixels.data();
    const size_t traced_floats = (size_t)lw * lh * 3;
    vk_render_params rp{};
    rp.width = lw; rp.height = lh; rp.samples_per_pixel = spp; rp.max_depth = depth; rp.seed = seed + 1;
    rp.integrator = integ; rp.background = bg; rp.background_color[0] = bgc[0]; rp.background_color[1] = bgc[1];
    rp.background_color[2] = bgc[2];
    rp.tile_rank = 0; rp.tile_world = 1;
    vk_temporal *history = nullptr;
    if (temporal) {
        vk_temporal_params tp;
        if (p_tp_defaults(width, height, &tp) != VK_OK || p_tcreate(scene, &tp, &history) != VK_OK) {
            fprintf(stderr, "vk_temporal_create: %s\n", p_err()); return 1; }
    }
    vk_tone *tone = nullptr;
    if (display && p_tone_create(scene, width, height, &tone) != VK_OK) { fprintf(stderr, "vk_tone_create: %s\n", p_err()); return 1; }
    vk_glare *glare = nullptr;
    if (glare_pct && p_glare_create(scene, width, height, &glare) != VK_OK) { fprintf(stderr, "vk_glare_create: %s\n", p_err()); return 1; }
    vk_psf *psf = nullptr;
    if (psf_streaks) {
        std::vector<float> star((size_t)PSF_K * PSF_K * 3);
        if (p_psf_star(PSF_K, psf_streaks, 0.0f, 8.0f, 0.1f, star.data()) != VK_OK || p_psf_create(scene, width, height, PSF_K, &psf) != VK_OK ||
            p_psf_load(psf, PSF_K, star.data()) != VK_OK) { fprintf(stderr, "vk_psf: %s\n", p_err()); return 1; }
    }
    vk_upsample *upsampler = nullptr;
    if (scaled && p_up_create(scene, lw, lh, width, height, &upsampler) != VK_OK) { fprintf(stderr, "vk_upsample_create: %s\n", p_err()); return 1; }
    vk_camera cam;
    int file_idx = 0;
    while (file_idx < frames && vkh_scene_next_camera(hs, &cam)) {   // main.rs:176
        auto start = std::chrono::steady_clock::now();
        if (temporal) rp.seed = seed + 1 + (uint64_t)file_idx;        // independent frames
        vk_stats st{};
        std::vector<float> err;                                       // the final standard error (steps >= 2)
        if (steps == 1) {
            if (p_render(scene, &cam, &rp, traced, &st) != VK_OK) { fprintf(stderr, "vk_render: %s\n", p_err()); return 1; }
        } else {
            vk_progress *pr = nullptr;
            if (p_pcreate(scene, &cam, &rp, VK_PROGRESS_STDERR, &pr) != VK_OK) { fprintf(stderr, "vk_progress_create: %s\n", p_err()); return 1; }
            err.resize(traced_floats);
            uint32_t done = 0;
            for (uint32_t k = 0; k < steps; k++) {
                const uint32_t n = (uint32_t)((uint64_t)spp * (k + 1) / steps) - done;
                vk_stats sw{};
                if (p_pstep(pr, n, traced, &sw) != VK_OK) { fprintf(stderr, "vk_progress_step: %s\n", p_err()); return 1; }
                done += n;
                st.samples += sw.samples; st.kernel_ms += sw.kernel_ms; st.kernel_launches += sw.kernel_launches;
                char sfn[64];
                snprintf(sfn, sizeof sfn, "output_%04d_step%02u.ppm", file_idx, k);
                if (vkh_write_ppm(sfn, traced, lw, lh)) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
                // mean relative standard error over the pixel components with a non-zero mean (needs two windows)
                double rel = 0.0; size_t cnt = 0;
                if (k >= 1) {
                    if (p_pstderr(pr, err.data()) != VK_OK) { fprintf(stderr, "vk_progress_stderr: %s\n", p_err()); return 1; }
                    for (size_t i = 0; i < traced_floats; i++)
                        if (traced[i] > 0.0f && std::isfinite(err[i])) { rel += (double)err[i] / (double)traced[i]; cnt++; }
                }
                if (k >= 1) fprintf(stderr, "  %s: %u/%u samples, mean relative standard error %.4f\n", sfn, done, spp, cnt ? rel / (double)cnt : 0.0);
                else fprintf(stderr, "  %s: %u/%u samples, mean relative standard error n/a (one window)\n", sfn, done, spp);
            }
            p_pdestroy(pr);
        }
        char fn[64];
        snprintf(fn, sizeof fn, "output_%04d.ppm", file_idx);         // main.rs:201
        if (vkh_write_ppm(fn, traced, lw, lh)) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
        std::vector<float> shown;                                     // the last stage's float frame (display): empty = `pixels`
        if (aov_spp > 0) {
            const size_t np = (size_t)width * height;
            std::vector<float> albedo(np * 3), normal(np * 3), zdepth(np), coverage(np);
            vk_render_params ap = rp;
            ap.width = width; ap.height = height; ap.samples_per_pixel = aov_spp;
            vk_stats as{};
            if (p_aov(scene, &cam, &ap, 0, albedo.data(), normal.data(), zdepth.data(), coverage.data(), &as) != VK_OK) {
                fprintf(stderr, "vk_render_aov: %s\n", p_err()); return 1; }
            const struct { const char *suffix; const float *data; int ch; } outs[] = {
                {"", traced, 3}, {"_albedo", albedo.data(), 3}, {"_normal", normal.data(), 3}, {"_depth", zdepth.data(), 1},
                {"_coverage", coverage.data(), 1}};
            for (const auto &o : outs) {
                char pfn[64];
                snprintf(pfn, sizeof pfn, "output_%04d%s.pfm", file_idx, o.suffix);
                if (!write_pfm(pfn, o.data, o.data == traced ? lw : width, o.data == traced ? lh : height, o.ch)) return 1;
            }
            fprintf(stderr, "  first-hit buffers of %u samples per pixel: kernel %.2f ms\n", aov_spp, as.kernel_ms);
            if (scaled) {
                // the same samples' first-hit buffers at the low size, then the low frame (and its standard error) to full size: from here
                // on `pixels` and `err` are full-size images
                const size_t nl = (size_t)lw * lh;
                std::vector<float> lalbedo(nl * 3), lnormal(nl * 3), ldepth(nl), err_hi(err.empty() ? 0 : np * 3);
                vk_render_params lp = ap;
                lp.width = lw; lp.height = lh;
                vk_stats ls{};
                vk_upsample_params up;
                vk_upsample_info ui{};
                if (p_aov(scene, &cam, &lp, 0, lalbedo.data(), lnormal.data(), ldepth.data(), nullptr, &ls) != VK_OK) {
                    fprintf(stderr, "vk_render_aov: %s\n", p_err()); return 1; }
                const struct { const char *suffix; const float *data; int ch; } louts[] = {
                    {"_lo_albedo", lalbedo.data(), 3}, {"_lo_normal", lnormal.data(), 3}, {"_lo_depth", ldepth.data(), 1}};
                for (const auto &o : louts) {
                    char pfn[64];
                    snprintf(pfn, sizeof pfn, "output_%04d%s.pfm", file_idx, o.suffix);
                    if (!write_pfm(pfn, o.data, lw, lh, o.ch)) return 1;
                }
                if (p_up_defaults(&up) != VK_OK ||
                    p_up_load(upsampler, traced, err.empty() ? nullptr : err.data(), lalbedo.data(), lnormal.data(), ldepth.data()) != VK_OK ||
                    p_up_apply(upsampler, &up, albedo.data(), normal.data(), zdepth.data(), pixels.data(), err.empty() ? nullptr : err_hi.data()) != VK_OK ||
                    p_up_info(upsampler, &ui) != VK_OK) {
                    fprintf(stderr, "vk_upsample: %s\n", p_err()); return 1; }
                if (!err.empty()) err.swap(err_hi);
                char ufn[64];
                snprintf(ufn, sizeof ufn, "output_%04d_upsampled.ppm", file_idx);
                if (vkh_write_ppm(ufn, pixels.data(), width, height)) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
                snprintf(ufn, sizeof ufn, "output_%04d_upsampled.pfm", file_idx);
                if (!write_pfm(ufn, pixels.data(), width, height, 3)) return 1;
                fprintf(stderr, "  upsampled %u x %u to %u x %u: kernel %.2f ms, %llu pixels by the tent alone, %llu empty\n", lw, lh, width, height,
                        ui.last_kernel_ms, (unsigned long long)ui.fallback_pixels, (unsigned long long)ui.empty_pixels);
            }
            // what the temporal and denoise steps are guided by: the first-hit buffers, or the specular guides
            const float *g_albedo = albedo.data(), *g_normal = normal.data(), *g_depth = zdepth.data();
            std::vector<float> galbedo, gnormal, gdepth, gbounces;
            if (guide_bounces > 0) {
                galbedo.resize(np * 3); gnormal.resize(np * 3); gdepth.resize(np); gbounces.resize(np);
                vk_guide_params gp;
                vk_stats gs{};
                if (p_gp_defaults(&gp) != VK_OK) { fprintf(stderr, "vk_guide_default_params: %s\n", p_err()); return 1; }
                gp.max_bounces = guide_bounces;
                if (p_guides(scene, &cam, &ap, 0, &gp, galbedo.data(), gnormal.data(), gdepth.data(), nullptr, gbounces.data(), &gs) != VK_OK) {
                    fprintf(stderr, "vk_render_guides: %s\n", p_err()); return 1; }
                const struct { const char *suffix; const float *data; int ch; } gouts[] = {
                    {"_guide_albedo", galbedo.data(), 3}, {"_guide_normal", gnormal.data(), 3}, {"_guide_depth", gdepth.data(), 1},
                    {"_guide_bounces", gbounces.data(), 1}};
                for (const auto &o : gouts) {
                    char pfn[64];
                    snprintf(pfn, sizeof pfn, "output_%04d%s.pfm", file_idx, o.suffix);
                    if (!write_pfm(pfn, o.data, width, height, o.ch)) return 1;
                }
                fprintf(stderr, "  specular guides, at most %u bounces: kernel %.2f ms\n", guide_bounces, gs.kernel_ms);
                g_albedo = galbedo.data(); g_normal = gnormal.data(); g_depth = gdepth.data();
            }
            const float *dn_color = pixels.data(), *dn_err = err.data();
            std::vector<float> acc, acc_err;
            if (temporal) {
                acc.resize(np * 3); acc_err.resize(np * 3);
                vk_stats ts{};
                vk_temporal_info ti{};
                if (p_taccum(history, &cam, pixels.data(), err.data(), g_albedo, g_normal, g_depth, acc.data(), acc_err.data(),
                             nullptr, &ts) != VK_OK || p_tinfo(history, &ti) != VK_OK) {
                    fprintf(stderr, "vk_temporal_accumulate: %s\n", p_err()); return 1; }
                char tfn[64];
                snprintf(tfn, sizeof tfn, "output_%04d_temporal.ppm", file_idx);
                if (vkh_write_ppm(tfn, acc.data(), width, height)) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
                snprintf(tfn, sizeof tfn, "output_%04d_temporal.pfm", file_idx);
                if (!write_pfm(tfn, acc.data(), width, height, 3)) return 1;
                fprintf(stderr, "  accumulated: %.1f %% of the pixels with history, kernel %.2f ms\n",
                        100.0 * (double)ti.pixels_with_history / (double)np, ts.kernel_ms);
                dn_color = acc.data(); dn_err = acc_err.data();
                if (display || glare || psf) shown = acc;
            }
            if (denoise) {
                vk_denoise_params dp;
                std::vector<float> clean(np * 3);
                vk_stats ds{};
                if (p_dn_defaults(width, height, &dp) != VK_OK ||
                    p_denoise(scene, &dp, dn_color, dn_err, g_albedo, g_normal, g_depth, clean.data(), &ds) != VK_OK) {
                    fprintf(stderr, "vk_denoise: %s\n", p_err()); return 1; }
                char dfn[64];
                snprintf(dfn, sizeof dfn, "output_%04d_denoised.ppm", file_idx);
                if (vkh_write_ppm(dfn, clean.data(), width, height)) { fprintf(stderr, "%s\n", vkh_last_error()); return 1; }
                snprintf(dfn, sizeof dfn, "output_%04d_denoised.pfm", file_idx);
                if (!write_pfm(dfn, clean.data(), width, height, 3)) return 1;
                fprintf(stderr, "  denoised (%u levels): kernels %.2f ms\n", dp.levels, ds.kernel_ms);
                if (display || glare || psf) shown = clean;
            }
        }
        if (glare) {
            vk_glare_params gp;
            if (shown.empty()) shown = pixels;
            if (p_glare_defaults(&gp) != VK_OK) { fprintf(stderr, "vk_glare defaults: %s\n", p_err()); return 1; }
            gp.strength = (float)glare_pct / 100.0f;
            if (p_glare_apply(glare, &gp, shown.data(), shown.data()) != VK_OK) { fprintf(stderr, "vk_glare_apply: %s\n", p_err()); return 1; }
            char sfn[64];
            snprintf(sfn, sizeof sfn, "output_%04d_glare.pfm", file_idx);
            if (!write_pfm(sfn, shown.data(), width, height, 3)) return 1;
            fprintf(stderr, "  glare: strength %.2f over %u levels\n", (double)gp.strength, gp.levels);
        }
        if (psf) {
            vk_psf_params pp;
            if (shown.empty()) shown = pixels;
            if (p_psf_defaults(&pp) != VK_OK) { fprintf(stderr, "vk_psf defaults: %s\n", p_err()); return 1; }
            if (p_psf_apply(psf, &pp, shown.data(), shown.data()) != VK_OK) { fprintf(stderr, "vk_psf_apply: %s\n", p_err()); return 1; }
            char sfn[64];
            snprintf(sfn, sizeof sfn, "output_%04d_psf.pfm", file_idx);
            if (!write_pfm(sfn, shown.data(), width, height, 3)) return 1;
            fprintf(stderr, "  psf: a star of %u streaks, %u x %u, strength %.2f\n", psf_streaks, PSF_K, PSF_K, (double)pp.strength);
        }
        if (display) {
            vk_tone_meter_params mp;
            vk_tone_params tp;
            vk_tone_meter_info mi{};
            std::vector<uint8_t> codes((size_t)width * height * 3);
            if (p_tone_mdefaults(&mp) != VK_OK || p_tone_defaults(&tp) != VK_OK) { fprintf(stderr, "vk_tone defaults: %s\n", p_err()); return 1; }
            if (frames > 1) mp.blend = 0.25f;
            tp.curve = display == 1 ? VK_TONE_REINHARD : display == 2 ? VK_TONE_HABLE : VK_TONE_ACES;
            if (p_tone_load(tone, shown.empty() ? pixels.data() : shown.data()) != VK_OK || p_tone_meter(tone, &mp, &mi) != VK_OK ||
                p_tone_encode(tone, &tp, codes.data()) != VK_OK) {
                fprintf(stderr, "vk_tone: %s\n", p_err()); return 1; }
            char sfn[64];
            snprintf(sfn, sizeof sfn, "output_%04d_display.ppm", file_idx);
            if (!write_ppm_codes(sfn, codes.data(), width, height)) return 1;
            fprintf(stderr, "  display: exposure %.4g (log2 luminance %.3f, target %.3f)\n", (double)mi.exposure, mi.log2_used, mi.log2_target);
        }
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        fprintf(stderr, "Wrote frame %s in %.3fs (kernel %.1f ms, %.1f Msamples/s)\n", fn, secs, st.kernel_ms,
                st.kernel_ms > 0 ? (double)st.samples / st.kernel_ms / 1e3 : 0.0);   // main.rs:215
        file_idx++;
    }
    if (upsampler) p_up_destroy(upsampler);
    if (psf) p_psf_destroy(psf);
    if (glare) p_glare_destroy(glare);
    if (tone) p_tone_destroy(tone);
    if (history) p_tdestroy(history);
    p_destroy(scene);
    vkh_scene_free(hs);
    return 0;
}
