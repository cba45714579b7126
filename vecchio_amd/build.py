"""Build recipes (explicit hipcc / g++ command lines, outputs in-tree so they travel with gpurun).

-ffp-contract=off everywhere: the reference's f32 arithmetic is unfused (Rust never
contracts a*b+c) and host/device parity of every control-flow value depends on it.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vecchio_amd", "csrc")
HOST = os.path.join(ROOT, "vecchio_amd", "host")
LIB = os.path.join(ROOT, "vecchio_amd", "lib")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = os.environ.get("CXX", "g++")
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra"]
# -fno-slp-vectorize: left alone, LLVM packs adjacent scalar f32 adds/multiplies of the sphere test and the shading code into
# v_pk_add_f32 / v_pk_mul_f32 behind v_mov shuffles and s_nops; on gfx950 those do not issue faster than the scalar pair and cost
# registers (measured: C2 +2.3 %, C4 +2.4 %, C3 +7.8 %, C5 +2.3 % without them; the sphere-only kernel 78 -> 74 VGPRs)
HIPFLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-fPIC",
            "-Wall", "-Wno-unused-function"]


def _fingerprint(sources, flags=()):
    """content hash of the sources (and the flags they are built with): what a built file is a function of"""
    import hashlib
    h = hashlib.sha256(" ".join(flags).encode())
    for s in sorted(sources):
        h.update(os.path.basename(s).encode())
        with open(s, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _newer(target, sources, flags=()):
    """Is `target` stale?  By CONTENT, not by mtime: every built file has a `<file>.src` stamp beside it holding the hash of
    the sources it was built from, so a library pushed to another machine (gpurun copies the tree; timestamps mean nothing
    there) is rebuilt exactly when it is not the build of the sources next to it."""
    stamp = target + ".src"
    if not os.path.exists(target) or not os.path.exists(stamp):
        return True
    with open(stamp) as f:
        return f.read().strip() != _fingerprint(sources, flags)


def _stamp(target, sources, flags=()):
    with open(target + ".src", "w") as f:
        f.write(_fingerprint(sources, flags) + "\n")


def _run(cmd):
    print("+", " ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)


def _run_atomic(cmd_before_out, out, cmd_after_out):
    """compile to a temporary name, then rename into place: a concurrent loader never sees a half-written file"""
    tmp = f"{out}.tmp.{os.getpid()}"
    try:
        _run(cmd_before_out + [tmp] + cmd_after_out)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _host_deps():
    srcs = [os.path.join(HOST, f) for f in ("host.cpp", "scene.cpp", "host_api.cpp")]
    return srcs, srcs + [os.path.join(HOST, "vecchio_host.hpp"), os.path.join(HOST, "host_api.h"),
                         os.path.join(CSRC, "vk_math.h"), os.path.join(ROOT, "include", "vecchio_amd.h")]


def _device_deps():
    srcs = [os.path.join(CSRC, "vk_api.hip"), os.path.join(CSRC, "vk_linearize.cpp")]
    return srcs, srcs + [os.path.join(CSRC, f) for f in ("vk_kernels.h", "vk_trace.h", "vk_math.h", "vk_device_scene.h", "vk_linearize.h", "vk_resources.h",
                                                         "vk_emit.h", "vk_adapt.h", "vk_adapt.hip", "vk_splat.h", "vk_splat.hip", "vk_matte.h",
                                                         "vk_matte.hip", "vk_robust.h", "vk_robust.hip", "vk_lpe.h", "vk_lpe.hip", "vk_tone.h", "vk_tone.hip",
                                                         "vk_nlm.h", "vk_nlm.hip", "vk_glare.h", "vk_glare.hip", "vk_upsample.h", "vk_upsample.hip", "vk_psf.h", "vk_psf.hip")] + \
        [os.path.join(ROOT, "include", "vecchio_amd.h"), os.path.join(ROOT, "include", "vecchio_amd_debug.h")]


def host_is_stale():
    return _newer(os.path.join(LIB, "libvecchio_host.so"), _host_deps()[1], CXXFLAGS)


def device_is_stale():
    return _newer(os.path.join(LIB, "libvecchio_amd.so"), _device_deps()[1], HIPFLAGS) or not os.path.exists(kernel_resources_path()) or \
        not os.path.exists(kernel_resources_adapt_path()) or not os.path.exists(kernel_resources_splat_path()) or \
        not os.path.exists(kernel_resources_matte_path()) or not os.path.exists(kernel_resources_robust_path()) or \
        not os.path.exists(kernel_resources_lpe_path()) or not os.path.exists(kernel_resources_tone_path()) or \
        not os.path.exists(kernel_resources_nlm_path()) or not os.path.exists(kernel_resources_glare_path()) or \
        not os.path.exists(kernel_resources_upsample_path()) or not os.path.exists(kernel_resources_psf_path())


def build_host(force=False):
    out = os.path.join(LIB, "libvecchio_host.so")
    srcs, deps = _host_deps()
    if force or _newer(out, deps, CXXFLAGS):
        os.makedirs(LIB, exist_ok=True)
        _run_atomic([CXX] + CXXFLAGS + ["-shared", "-o"], out, srcs + ["-lz"])   # zlib: the decoded texture images are .ppm.gz
        _stamp(out, deps, CXXFLAGS)
    return out


def build_cli(force=False):
    out = os.path.join(LIB, "vecchio_cli")
    src = os.path.join(HOST, "main.cpp")
    if not os.path.exists(src):
        return None
    host = build_host()
    deps = [src, os.path.join(HOST, "host_api.h"), os.path.join(ROOT, "include", "vecchio_amd.h")]
    if force or _newer(out, deps, CXXFLAGS) or not os.path.exists(host):
        _run([CXX] + CXXFLAGS + ["-o", out, src, "-L" + LIB, "-lvecchio_host", "-ldl", "-Wl,-rpath,$ORIGIN"])
        _stamp(out, deps, CXXFLAGS)
    return out


def build_device_debug(force=False):
    """libvecchio_amd_debug.so: the product library's sources with -DVK_DEBUG_LIB — plus the instrumented (STATS) kernel builds behind
    vk_debug_phase_stats and the device arithmetic probe vk_debug_math (include/vecchio_amd_debug.h).  Tests and diagnostics only:
    the product library holds production kernels only."""
    out = os.path.join(LIB, "libvecchio_amd_debug.so")
    srcs, deps = _device_deps()
    flags = HIPFLAGS + ["-DVK_DEBUG_LIB"]
    if force or _newer(out, deps, flags):
        os.makedirs(LIB, exist_ok=True)
        _run_atomic([HIPCC] + flags + ["-shared", "-o"], out, srcs + [_adapt_src(), _splat_src(), _matte_src(), _robust_src(), _lpe_src(), _tone_src(), _nlm_src(), _glare_src(), _upsample_src(), _psf_src()])
        _stamp(out, deps, flags)
    return out


def debug_is_stale():
    return _newer(os.path.join(LIB, "libvecchio_amd_debug.so"), _device_deps()[1], HIPFLAGS + ["-DVK_DEBUG_LIB"])


def _adapt_src():
    """the kernels of vk_adapt_* (films: error moments and tile runs): a translation unit of its own"""
    return os.path.join(CSRC, "vk_adapt.hip")


def _splat_src():
    """the kernels of vk_splat_* (reconstruction filters: the splat of a path batch and its resolve): a translation unit of its own"""
    return os.path.join(CSRC, "vk_splat.hip")


def _matte_src():
    """the kernels of vk_render_mattes (ID mattes: a ranked table of object or material ids per pixel): a translation unit of its own"""
    return os.path.join(CSRC, "vk_matte.hip")


def _robust_src():
    """the kernels of vk_robust_* (robust film: the bucketed deposit of a path batch and its trimmed resolve): a translation unit of its own"""
    return os.path.join(CSRC, "vk_robust.hip")


def _lpe_src():
    """the kernels of vk_lpe_* (light-path layers: a path's tag per bounce, the layered deposit of a path batch and a layer's resolve): a
    translation unit of its own"""
    return os.path.join(CSRC, "vk_lpe.hip")


def _tone_src():
    """the kernels of vk_tone_* (display transform: a frame's luminance histogram and its encoding to 8-bit codes): a translation unit of
    its own"""
    return os.path.join(CSRC, "vk_tone.hip")


def _nlm_src():
    """the kernels of vk_nlm_* (non-local means: the prepare pass into the handle's planes and the filter in its two forms): a translation
    unit of its own"""
    return os.path.join(CSRC, "vk_nlm.hip")


def _glare_src():
    """the kernels of vk_glare_* (glare: the down passes of the bright part's pyramid in their plain and LDS forms, the tail, the up
    pass and the composite): a translation unit of its own"""
    return os.path.join(CSRC, "vk_glare.hip")


def _upsample_src():
    """the kernels of vk_upsample_* (guided upsampling: the prepare pass over the low frame and the filter over the high one in its
    plain and tiled forms): a translation unit of its own"""
    return os.path.join(CSRC, "vk_upsample.hip")


def _psf_src():
    """the kernels of vk_psf_* (point-spread function: the pad, place, bit-reversal, stage, product, scale and composite kernels of the
    plain form and the line kernel of the LDS form): a translation unit of its own"""
    return os.path.join(CSRC, "vk_psf.hip")


def _hipcc_with_remarks(cmd, cwd, cleanup=()):
    """runs a hipcc line that carries -Rpass-analysis=kernel-resource-usage and -save-temps in `cwd`: (the remark lines, kernel symbol ->
    scratch instructions from the gfx950 assembly it left there); everything else it wrote to stderr is passed on"""
    print("+", " ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, cwd=cwd)
    remarks = [l for l in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" in l]
    other = [l for l in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in l]
    if other:
        print("\n".join(other), file=sys.stderr)
    if r.returncode != 0:
        for f in cleanup:
            if os.path.exists(f):
                os.remove(f)
        raise subprocess.CalledProcessError(r.returncode, cmd)
    spills = {}
    for f in os.listdir(cwd):
        if f.endswith("gfx950.s"):
            spills.update(_scratch_ops(open(os.path.join(cwd, f)).read()))
    return remarks, spills


def _write_resources(path, remarks, spills):
    """registers / scratch / occupancy of every kernel, kept next to the library: the megakernel's
    throughput collapses when a variant starts spilling, so tests/test_kernel_resources.py pins them.
    ScratchOps = number of scratch_load/scratch_store instructions in the kernel's code: the remark's
    ScratchSize does not move when the allocator spills the same slots in twice as many places."""
    text = "\n".join(re.sub(r"^.*remark: [^ ]* ", "", l).replace(" [-Rpass-analysis=kernel-resource-usage]", "") for l in remarks) + "\n"
    blocks = text.split("Function Name: ")
    text = blocks[0] + "".join("Name: " + b.rstrip("\n") + f"\n   ScratchOps: {spills.get(b.split()[0], -1)}\n" for b in blocks[1:])
    with open(path, "w") as f:
        f.write(text)


def build_device(force=False):
    """hipcc cross-compiles for gfx950 without a GPU present.  Eleven steps: vk_adapt.hip, vk_splat.hip, vk_matte.hip, vk_robust.hip,
    vk_lpe.hip, vk_tone.hip, vk_nlm.hip, vk_glare.hip, vk_upsample.hip and vk_psf.hip (kernel_resources_psf.txt) to an object of their own each (their resource remarks go to kernel_resources_adapt.txt,
    kernel_resources_splat.txt, kernel_resources_matte.txt, kernel_resources_robust.txt, kernel_resources_lpe.txt,
    kernel_resources_tone.txt, kernel_resources_nlm.txt, kernel_resources_glare.txt and kernel_resources_upsample.txt), then vk_api.hip and vk_linearize.cpp, linked with those objects (kernel_resources.txt: theirs alone)."""
    out = os.path.join(LIB, "libvecchio_amd.so")
    srcs, deps = _device_deps()
    if force or device_is_stale():
        os.makedirs(LIB, exist_ok=True)
        # -save-temps in a scratch directory: the gfx950 assembly is read back for the per-kernel spill counts
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            analysis = ["-Rpass-analysis=kernel-resource-usage", "-save-temps"]
            tmp_adapt, tmp_splat, tmp_main = os.path.join(tmp, "adapt"), os.path.join(tmp, "splat"), os.path.join(tmp, "main")
            tmp_matte, tmp_robust = os.path.join(tmp, "matte"), os.path.join(tmp, "robust")
            os.makedirs(tmp_adapt)
            os.makedirs(tmp_splat)
            os.makedirs(tmp_matte)
            os.makedirs(tmp_robust)
            tmp_lpe = os.path.join(tmp, "lpe")
            os.makedirs(tmp_lpe)
            tmp_tone = os.path.join(tmp, "tone")
            os.makedirs(tmp_tone)
            os.makedirs(tmp_main)
            adapt_obj = os.path.join(tmp_adapt, "vk_adapt.o")
            adapt = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", adapt_obj, _adapt_src()], tmp_adapt)
            splat_obj = os.path.join(tmp_splat, "vk_splat.o")
            splat = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", splat_obj, _splat_src()], tmp_splat)
            matte_obj = os.path.join(tmp_matte, "vk_matte.o")
            matte = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", matte_obj, _matte_src()], tmp_matte)
            robust_obj = os.path.join(tmp_robust, "vk_robust.o")
            robust = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", robust_obj, _robust_src()], tmp_robust)
            lpe_obj = os.path.join(tmp_lpe, "vk_lpe.o")
            lpe = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", lpe_obj, _lpe_src()], tmp_lpe)
            tone_obj = os.path.join(tmp_tone, "vk_tone.o")
            tone = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", tone_obj, _tone_src()], tmp_tone)
            tmp_nlm = os.path.join(tmp, "nlm")
            os.makedirs(tmp_nlm)
            nlm_obj = os.path.join(tmp_nlm, "vk_nlm.o")
            nlm = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", nlm_obj, _nlm_src()], tmp_nlm)
            tmp_glare = os.path.join(tmp, "glare")
            os.makedirs(tmp_glare)
            glare_obj = os.path.join(tmp_glare, "vk_glare.o")
            glare = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", glare_obj, _glare_src()], tmp_glare)
            tmp_upsample = os.path.join(tmp, "upsample")
            os.makedirs(tmp_upsample)
            upsample_obj = os.path.join(tmp_upsample, "vk_upsample.o")
            upsample = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", upsample_obj, _upsample_src()], tmp_upsample)
            tmp_psf = os.path.join(tmp, "psf")
            os.makedirs(tmp_psf)
            psf_obj = os.path.join(tmp_psf, "vk_psf.o")
            psf = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-c", "-o", psf_obj, _psf_src()], tmp_psf)
            tmp_out = f"{out}.tmp.{os.getpid()}"
            # (the objects in front of the sources: hipcc reads whatever follows a source file as HIP)
            main = _hipcc_with_remarks([HIPCC] + HIPFLAGS + analysis + ["-shared", "-o", tmp_out, adapt_obj, splat_obj, matte_obj, robust_obj, lpe_obj, tone_obj, nlm_obj, glare_obj, upsample_obj, psf_obj] + srcs, tmp_main, [tmp_out])
            os.replace(tmp_out, out)
        _write_resources(kernel_resources_path(), *main)
        _write_resources(kernel_resources_adapt_path(), *adapt)
        _write_resources(kernel_resources_splat_path(), *splat)
        _write_resources(kernel_resources_matte_path(), *matte)
        _write_resources(kernel_resources_robust_path(), *robust)
        _write_resources(kernel_resources_lpe_path(), *lpe)
        _write_resources(kernel_resources_tone_path(), *tone)
        _write_resources(kernel_resources_nlm_path(), *nlm)
        _write_resources(kernel_resources_glare_path(), *glare)
        _write_resources(kernel_resources_upsample_path(), *upsample)
        _write_resources(kernel_resources_psf_path(), *psf)
        _stamp(out, deps, HIPFLAGS)
    return out


def _scratch_ops(asm):
    """kernel symbol -> number of scratch_* instructions between its label and .Lfunc_end"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M):
        out[m.group(1)] = sum(1 for l in m.group(2).split("\n") if l.lstrip().startswith("scratch_"))
    return out


def kernel_resources_path():
    return os.path.join(LIB, "kernel_resources.txt")


def kernel_resources_adapt_path():
    """the same record for the kernels of vk_adapt.hip"""
    return os.path.join(LIB, "kernel_resources_adapt.txt")


def kernel_resources_splat_path():
    """the same record for the kernels of vk_splat.hip"""
    return os.path.join(LIB, "kernel_resources_splat.txt")


def kernel_resources_matte_path():
    """the same record for the kernels of vk_matte.hip"""
    return os.path.join(LIB, "kernel_resources_matte.txt")


def kernel_resources_robust_path():
    """the same record for the kernels of vk_robust.hip"""
    return os.path.join(LIB, "kernel_resources_robust.txt")


def kernel_resources_lpe_path():
    """the same record for the kernels of vk_lpe.hip"""
    return os.path.join(LIB, "kernel_resources_lpe.txt")


def kernel_resources_tone_path():
    """the same record for the kernels of vk_tone.hip"""
    return os.path.join(LIB, "kernel_resources_tone.txt")


def kernel_resources_nlm_path():
    """the same record for the kernels of vk_nlm.hip"""
    return os.path.join(LIB, "kernel_resources_nlm.txt")


def kernel_resources_glare_path():
    """the same record for the kernels of vk_glare.hip"""
    return os.path.join(LIB, "kernel_resources_glare.txt")


def kernel_resources_upsample_path():
    """the same record for the kernels of vk_upsample.hip"""
    return os.path.join(LIB, "kernel_resources_upsample.txt")


def kernel_resources_psf_path():
    """the same record for the kernels of vk_psf.hip"""
    return os.path.join(LIB, "kernel_resources_psf.txt")


def build_oracle(force=False):
    """CPU oracle (test infrastructure).  oracle/_ref does not exist: the reference is Rust and
    there is no cargo/rustc in this image."""
    odir = os.path.join(ROOT, "oracle")
    out = os.path.join(odir, "_build", "liboracle.so")
    deps = [os.path.join(odir, "oracle.cpp"), os.path.join(odir, "oracle.h"), os.path.join(CSRC, "vk_math.h"),
            os.path.join(ROOT, "include", "vecchio_amd.h")]
    if force or _newer(out, deps, ("oracle",)):
        _run(["make", "-B", "-C", odir])
        _stamp(out, deps, ("oracle",))
    return out


def build_emu(force=False):
    """Test-only host build of the kernel's per-lane logic (tests/emu)."""
    edir = os.path.join(ROOT, "tests", "emu")
    out = os.path.join(edir, "_build", "libemu.so")
    srcs = [os.path.join(edir, "emu.cpp"), os.path.join(edir, "emu_guides.cpp"), os.path.join(edir, "emu_rays.cpp"),
            os.path.join(edir, "emu_occlusion.cpp"), os.path.join(edir, "emu_radiance.cpp"),
            os.path.join(edir, "emu_irradiance.cpp"), os.path.join(edir, "emu_probes.cpp"), os.path.join(edir, "emu_shade.cpp"),
            os.path.join(edir, "emu_paths.cpp"), os.path.join(edir, "emu_film.cpp"), os.path.join(edir, "emu_adapt.cpp"),
            os.path.join(edir, "emu_splat.cpp"), os.path.join(edir, "emu_matte.cpp"), os.path.join(edir, "emu_robust.cpp"),
            os.path.join(edir, "emu_lpe.cpp"), os.path.join(edir, "emu_tone.cpp"), os.path.join(edir, "emu_nlm.cpp"),
            os.path.join(edir, "emu_glare.cpp"), os.path.join(edir, "emu_upsample.cpp"), os.path.join(edir, "emu_psf.cpp"),
            os.path.join(CSRC, "vk_linearize.cpp")]
    # (the tool's own headers: whichever are there)
    deps = srcs + sorted(os.path.join(edir, f) for f in os.listdir(edir) if f.endswith(".h")) + \
        [os.path.join(CSRC, f) for f in ("vk_trace.h", "vk_math.h", "vk_device_scene.h", "vk_linearize.h", "vk_adapt.h", "vk_splat.h", "vk_matte.h", "vk_robust.h", "vk_lpe.h", "vk_tone.h", "vk_nlm.h", "vk_glare.h", "vk_upsample.h", "vk_psf.h")] + \
        [os.path.join(ROOT, "include", "vecchio_amd.h"), os.path.join(ROOT, "include", "vecchio_amd_debug.h")]
    if force or _newer(out, deps, CXXFLAGS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        _run([CXX] + CXXFLAGS + ["-shared", "-o", out] + srcs + ["-lpthread"])
        _stamp(out, deps, CXXFLAGS)
    return out


def build_mock_rccl(force=False):
    """Test double of librccl.so (tests/mock_rccl): the library's RCCL gather on a one-GPU box, through the DEBUG build only."""
    mdir = os.path.join(ROOT, "tests", "mock_rccl")
    out = os.path.join(mdir, "_build", "librccl_mock.so")
    src = os.path.join(mdir, "mock_rccl.cpp")
    flags = ["-O2", "-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    if force or _newer(out, [src], flags):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        _run([CXX] + flags + ["-shared", "-o", out, src, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
        _stamp(out, [src], flags)
    return out


def build_all(force=False):
    return [build_host(force), build_device(force), build_device_debug(force), build_oracle(force), build_emu(force), build_cli(force),
            build_mock_rccl(force)]


if __name__ == "__main__":
    build_all("--force" in sys.argv)
