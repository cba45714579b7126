"""Films (vk_film_*): a frame from a path batch with the camera and the frame sums on the device, next to the route they replace — rays
and states made on the host, vk_paths_begin, vk_paths_results, the fixed-point sums in numpy — and next to vk_render.  Writes
profiles/film/report.jsonl (one JSON line per case) and prints them.

    python tools/film_report.py [--repeats 3] [--cases c2,cornell,final,forms] [--out profiles/film/report.jsonl]

Frames: those of tools/paths_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — at one path per pixel,
max_depth 50, the scene's own integrator and background.  After a warm-up of each, three routes run interleaved in one process,
--repeats times, every value kept and the median reported:
  (a) the host route: pixel-centre rays and path states built in numpy (timed apart: wall seconds are given with and without it),
      PathBatch.begin, step until nothing is live, results(), then the finite filter, the clamp and the 2^-26 sums in numpy (the part
      up to and including results() is given too: the route without any arithmetic of the caller's);
  (b) the film route: Film.emit of the whole frame, step until nothing is live, Film.deposit, Film.resolve to the host;
  (c) vk_render of the same frame at one sample per pixel, for orientation; whether (b)'s frame equals (c)'s bit for bit is reported.
Beside the emit, deposit and resolve milliseconds (vk_debug_film_last_ms) stand the batch's kernel_ms and a device-to-device copy of
the bytes each moves (emit: 84 a path written; deposit: 36 a path read and 24 added; resolve: 24 a pixel read and 12 written).
Case `forms`: the deposit in its two forms on C2's frame at 1 and at 8 samples per pixel (one emit of all of them), interleaved.
Nothing passes or fails.  Each case is a timed step of its own: a child process under a time limit; after one fails no further one is
started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 420
f32 = np.float32
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def host_sums(states, status, n_pixels, spp):
    """the render kernel's finite filter, clamp and 2^-26 sums in numpy, then resolve_kernel's arithmetic: (n_pixels, 3) float32"""
    acc = states["acc"]
    ok = np.isfinite(acc).all(axis=1) & np.isin(status, (0, 2, 4)) & (states["pixel"] < n_pixels)
    clampv = min(f32(1e10), f32(1.3e11) / f32(spp))
    big = np.abs(acc).max(axis=1, keepdims=True)
    v = np.where(big <= f32(31.999), acc, np.clip(acc, -clampv, clampv))
    fixed = np.trunc(np.where(ok[:, None], v, 0) * f32(2.0 ** 26)).astype(np.int64)
    sums = np.zeros((n_pixels, 3), np.int64)
    np.add.at(sums, states["pixel"][ok], fixed[ok])
    return ((sums.astype(f32) * f32(2.0 ** -26)) / f32(spp)).astype(f32)


def setup(key):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from trace_rays_report import CASES
    from vecchio_amd import DeviceScene, HostScene
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    return torch, name, w, h, hs, cam, DeviceScene(hs.desc)


def frame(key, repeats):
    torch, name, w, h, hs, cam, ds = setup(key)
    from shade_report import copy_ms
    from trace_rays_report import primary_rays
    from vecchio_amd.scene import PATH_STATE_DTYPE
    try:
        n = w * h
        q = hs.params(w, 1, 50, seed=2, height=h)
        kw = dict(max_depth=50, integrator=hs.integrator, background=hs.background, background_color=hs.background_color)
        pb = ds.paths(n)
        film = ds.film(cam, q)
        frame_buf = np.zeros((h, w, 3), f32)                        # the caller's frame buffer, kept from frame to frame

        def host_route():
            t0 = time.perf_counter()
            rays = np.ascontiguousarray(primary_rays(cam, w, h).reshape(-1))
            states = np.zeros(n, PATH_STATE_DTYPE)
            states["thr"], states["depth"], states["seed"], states["pixel"] = 1.0, 1, q.seed, np.arange(n, dtype=np.uint32)
            t1 = time.perf_counter()
            pb.begin(rays, states, **kw)
            st = pb.step(1 << 20)
            res, status = pb.results()
            t_res = time.perf_counter()
            img = host_sums(res, status, n, 1)
            t2 = time.perf_counter()
            return t2 - t0, t2 - t1, st.kernel_ms, t_res - t1, img

        def film_route():
            film.reset()
            t0 = time.perf_counter()
            film.emit(pb, 0, 0, w, h, 0, 1)
            st = pb.step(1 << 20)
            film.deposit(pb)
            img = film.resolve(out=frame_buf)
            t1 = time.perf_counter()
            return t1 - t0, st.kernel_ms, film.last_ms(), img

        def render():
            t0 = time.perf_counter()
            img, st = ds.render(cam, q)
            return time.perf_counter() - t0, st.kernel_ms, img

        host_route(); film_route(); render()                       # warm-up
        a, b, c = [], [], []
        same = True
        for _ in range(repeats):                                    # interleaved
            ra, rb, rc = host_route(), film_route(), render()
            a.append(ra[:4]); b.append(rb[:3]); c.append(rc[:2])
            same = same and bool(np.array_equal(rb[3].view(np.uint32), rc[2].view(np.uint32)))
            frame_buf[:] = 0
        inf = film.info()
        moved = {"emit": 84 * n, "deposit": 60 * n, "resolve": 36 * n}
        copies = {k: r4(copy_ms(torch, v, repeats)) for k, v in moved.items()}
        parts = {k: r4(x[2][j] for x in b) for j, k in enumerate(("emit", "deposit", "resolve"))}
        line = {"case": key, "scene": name, "width": w, "height": h, "paths": n, "repeats": repeats,
                "film_frame_equals_vk_render_bit_for_bit": same,
                "host_route_wall_s": round(med(x[0] for x in a), 4), "host_route_wall_s_all": r4(x[0] for x in a),
                "host_route_wall_without_ray_generation_s": round(med(x[1] for x in a), 4),
                "host_route_wall_without_ray_generation_s_all": r4(x[1] for x in a),
                "host_route_begin_step_results_only_s": round(med(x[3] for x in a), 4),
                "host_route_begin_step_results_only_s_all": r4(x[3] for x in a),
                "film_below_begin_step_results_only_in_every_repeat": bool(all(y[0] < x[3] for x, y in zip(a, b))),
                "host_route_kernel_ms": round(med(x[2] for x in a), 3), "host_route_kernel_ms_all": r4(x[2] for x in a),
                "film_route_wall_s": round(med(x[0] for x in b), 4), "film_route_wall_s_all": r4(x[0] for x in b),
                "film_route_batch_kernel_ms": round(med(x[1] for x in b), 3), "film_route_batch_kernel_ms_all": r4(x[1] for x in b),
                "film_below_host_route_in_every_repeat": bool(all(y[0] < x[1] for x, y in zip(a, b))),
                "film_wall_over_host_route": round(med(x[0] for x in b) / med(x[0] for x in a), 4),
                "film_wall_over_host_route_without_ray_generation": round(med(x[0] for x in b) / med(x[1] for x in a), 4),
                "render_wall_s": round(med(x[0] for x in c), 4), "render_wall_s_all": r4(x[0] for x in c),
                "render_kernel_ms": round(med(x[1] for x in c), 3), "render_kernel_ms_all": r4(x[1] for x in c),
                "deposited": int(inf.deposited), "dropped": int(inf.dropped), "clamped": int(inf.clamped)}
        for k in ("emit", "deposit", "resolve"):
            line.update({f"{k}_ms": round(med(parts[k]), 4), f"{k}_ms_all": parts[k], f"{k}_bytes": moved[k],
                         f"{k}_copy_ms": round(med(copies[k]), 4), f"{k}_copy_ms_all": copies[k],
                         f"{k}_over_copy": round(med(parts[k]) / med(copies[k]), 3)})
        print(json.dumps(line), flush=True)
        film.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def forms(repeats):
    """the deposit's two forms on C2's frame, at 1 and 8 samples per pixel, each measured behind an emit and a run to the end of its own"""
    torch, name, w, h, hs, cam, ds = setup("c2")
    from vecchio_amd import ffi
    try:
        out = {"case": "forms", "scene": name, "width": w, "height": h, "repeats": repeats}
        pb = ds.paths(w * h * 8)
        for spp in (1, 8):
            q = hs.params(w, spp, 50, seed=2, height=h)
            film = ds.film(cam, q)
            ms = {0: [], 1: []}
            sums = {}
            for rep in range(repeats + 1):                          # the first round is the warm-up
                for form in (ffi.VK_DEBUG_FILM_DEPOSIT_PLAIN, ffi.VK_DEBUG_FILM_DEPOSIT_RUNS):
                    film.reset()
                    film.debug_deposit_form(form)
                    film.emit(pb, 0, 0, w, h, 0, spp)
                    pb.step(1 << 20)
                    film.deposit(pb)
                    if rep:
                        ms[form].append(film.last_ms()[1])
                    else:
                        sums[form] = film.debug_sums().tobytes()
            out.update({f"spp{spp}_paths": w * h * spp, f"spp{spp}_plain_ms": round(med(ms[0]), 4), f"spp{spp}_plain_ms_all": r4(ms[0]),
                        f"spp{spp}_runs_ms": round(med(ms[1]), 4), f"spp{spp}_runs_ms_all": r4(ms[1]),
                        f"spp{spp}_runs_over_plain": round(med(ms[1]) / med(ms[0]), 4),
                        f"spp{spp}_runs_wins_beyond_the_spread": bool(max(ms[1]) < min(ms[0])),
                        f"spp{spp}_same_bytes": sums[0] == sums[1]})
            film.close()
        print(json.dumps(out), flush=True)
        pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final,forms")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    if args.child:
        forms(args.repeats) if args.child == "forms" else frame(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--out", args.out],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"case {key} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
            status = 1
            break
        got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode != 0:
            print(f"case {key} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            status = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
