"""The frames and parameter cases the upsampling tests share (test_upsample_emu.py on the CPU, test_gpu_upsample.py on the device): a
small analytic scene sampled at both sizes by the mapping's own convention — pixel x of an n-wide frame has its centre at u = (x + 0.5) /
(n - 1) —, with misses, bad pixels and a block of invalid ones.  TESTS ONLY."""
import itertools

import numpy as np

f32 = np.float32
# the shapes the laws were first checked on, and the degenerate ones
CPU_SIZES = [(7, 5, 16, 11), (8, 6, 16, 12), (5, 4, 37, 29), (9, 7, 9, 7), (2, 2, 5, 5), (9, 7, 31, 23), (2, 2, 2, 2), (13, 11, 40, 33)]


def guides(n_x, n_y):
    """albedo (n_y, n_x, 3), normal (n_y, n_x, 3), depth (n_y, n_x) of the analytic scene: a floor plane receding in v, a slanted wall
    right of u = 0.47 in front of it, a disc that is a miss (depth inf, normal 0), a checker albedo"""
    u = ((np.arange(n_x) + 0.5) / (n_x - 1))[None, :] * np.ones((n_y, 1))
    v = ((np.arange(n_y) + 0.5) / (n_y - 1))[:, None] * np.ones((1, n_x))
    wall = u > 0.47
    depth = np.where(wall, 1.5 + 0.8 * u, 4.0 + 2.0 * v)
    normal = np.where(wall[..., None], np.array([0.6, 0.0, 0.8]), np.array([0.0, 2.0, 0.0]))        # (the floor's is not unit)
    miss = (u - 0.25) ** 2 + (v - 0.7) ** 2 < 0.02
    depth = np.where(miss, np.inf, depth)
    normal = np.where(miss[..., None], 0.0, normal)
    chk = ((np.floor(u * 6) + np.floor(v * 5)) % 2).astype(bool)
    albedo = np.where(chk[..., None], np.array([0.8, 0.7, 0.6]), np.array([0.2, 0.25, 0.0]))         # (a zero: the floor's business)
    albedo = np.where(miss[..., None], 0.0, albedo)
    return albedo.astype(f32), normal.astype(f32), depth.astype(f32)


def frame(w, h, W, H, seed=0, bad=False, block=False):
    """dict: the low images color, stderr3, albedo, normal, depth and the high guides albedo_hi, normal_hi, depth_hi.  bad: a few low
    pixels with NaN or inf in colour or stderr3, a NaN depth and an inf normal in the guides at both sizes.  block: a block of invalid
    low pixels, 6 x 6 where the frame has room (so that some high pixel has no valid tap) and a whole invalid frame's worth otherwise."""
    rng = np.random.default_rng(1000 + seed)
    a, n, z = guides(w, h)
    A, N, Z = guides(W, H)
    irr = (0.5 + rng.random((h, w, 3))).astype(f32)
    color = (irr * a + f32(0.01) * rng.random((h, w, 3)).astype(f32)).astype(f32)
    se = (f32(0.05) * (0.2 + rng.random((h, w, 3))) * color).astype(f32)
    if bad:
        k = max(1, w * h // 12)
        ys, xs = rng.integers(0, h, k), rng.integers(0, w, k)
        vals = [np.nan, np.inf, -np.inf]
        for i, (y, x) in enumerate(zip(ys, xs)):
            (color if i % 2 == 0 else se)[y, x, i % 3] = vals[i % 3]
        z[rng.integers(0, h), rng.integers(0, w)] = np.nan
        n[rng.integers(0, h), rng.integers(0, w)] = np.inf
        Z[rng.integers(0, H), rng.integers(0, W)] = np.nan
        N[rng.integers(0, H), rng.integers(0, W), 1] = np.nan
        A[rng.integers(0, H), rng.integers(0, W), 2] = np.nan
    if block:
        if w >= 8 and h >= 7:
            color[h - 6:, w - 6:, 1] = np.nan
        else:
            color[..., 0] = np.inf
    return dict(color=color, stderr3=se, albedo=a, normal=n, depth=z, albedo_hi=A, normal_hi=N, depth_hi=Z)


def cases():
    """(id, frame keywords, which guides 'a' 'n' 'z', stderr3 on, parameters): every subset of guides with stderr3 on and off, bad pixels
    in half of them; sigma_z x squarings with all guides; the invalid block; another floor"""
    out = []
    subsets = ["".join(s) for r in range(4) for s in itertools.combinations("anz", r)]
    sig, sq = [0.5, 1.0, 4.0], [0, 3, 7]
    for i, g in enumerate(subsets):
        for se in (True, False):
            out.append((f"g{g or '0'}-se{int(se)}", dict(seed=i, bad=bool((i + se) % 2)), g, se,
                        dict(sigma_z=sig[i % 3], normal_squarings=sq[(i + se) % 3])))
    for s in sig:
        for q in sq:
            out.append((f"s{s}-q{q}", dict(seed=20), "anz", True, dict(sigma_z=s, normal_squarings=q)))
    out.append(("block", dict(seed=30, block=True), "anz", True, {}))
    out.append(("block-bad-plain", dict(seed=31, block=True, bad=True), "", True, {}))
    out.append(("floor", dict(seed=32), "anz", True, dict(albedo_floor=0.3)))
    out.append(("q10", dict(seed=33), "n", False, dict(normal_squarings=10)))
    return out


def arguments(fr, g, se):
    """the keyword arguments of upsample_ref.apply / emu_upsample_ffi.apply for a frame, a subset of guides and stderr3 on or off"""
    kw = dict(stderr3=fr["stderr3"] if se else None, want_stderr=se)
    if "a" in g:
        kw.update(albedo=fr["albedo"], albedo_hi=fr["albedo_hi"])
    if "n" in g:
        kw.update(normal=fr["normal"], normal_hi=fr["normal_hi"])
    if "z" in g:
        kw.update(depth=fr["depth"], depth_hi=fr["depth_hi"])
    return kw


def same(a, b):
    """bit for bit, a NaN's payload (and sign) aside"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
