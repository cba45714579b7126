"""What tests/test_roulette_ref.py, tests/test_gpu_roulette.py and tools/roulette_report.py share: the termination rule of a path batch
handle (vk_roulette_set, include/vecchio_amd.h) restated in numpy — its draw, its decision and the scale a continuing path gets —,
the edge throughputs the rule is tried on, and the unbiasedness experiment's frame, seeds, bounds and statistic."""
import numpy as np

from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32
SALT = 0x52D1E7A9C3B5F04B
RULES = ((2, 0.1, 0.8), (3, 0.05, 1.0))

# the unbiasedness experiment: measured on the CPU emulators as |z| 0.19, 0.67, 0.63 and, for the control, 25.5, 19.8, 16.2 (bounds 4
# and 8).  With another salt or draw these have to be measured again before the bounds are kept.
UNBIASED = dict(scene="cornell_box", width=16, height=16, spp=1024, max_depth=50, rule=RULES[0], seed_plain=5, seed_rule=6, seed_control=7,
                z_max=4.0, z_control_min=8.0)


def _mix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, pixel, sample, depth):
    """u of the rule for a path state: draw number `depth` (>= 1) of the stream rng_for_sample(seed ^ SALT, pixel, sample) — vk_math.h
    next_u32 at counter depth - 1, through gen_f32.  Arrays or scalars; float32."""
    with np.errstate(over="ignore"):
        seed = np.asarray(seed, np.uint64) ^ np.uint64(SALT)
        h = _mix64(seed + np.uint64(0x9E3779B97F4A7C15))
        key = _mix64(h ^ ((np.asarray(pixel, np.uint64) << np.uint64(32)) | np.asarray(sample, np.uint64)))
        ctr = np.asarray(depth, np.uint32)                     # the counter after the increment
        x = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32) + ctr * np.uint32(0x9E3779B9)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x21F0AAAD)
        x = x ^ (x >> np.uint32(15))
        x = x ^ (key >> np.uint64(32)).astype(np.uint32)
        x = x * np.uint32(0x735A2D97)
        x = x ^ (x >> np.uint32(15))
    return (x >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)


def q_of(thr, q_min, q_max):
    """the survival probability per path: fminf(fmaxf(max of the three components, NaNs dropped, q_min), q_max); thr (n, 3) float32"""
    thr = np.asarray(thr, f32).reshape(-1, 3)
    m = np.fmax(np.fmax(thr[:, 0], thr[:, 1]), thr[:, 2])
    return np.fmin(np.fmax(m, f32(q_min)), f32(q_max)).astype(f32)


def rule(states, first_depth, q_min, q_max):
    """(keep uint8, scale float32) per state, as vk_paths_cull takes them, of SCATTERED paths' states after a bounce: a state below
    first_depth is kept with scale 1 (thr * 1.0f is thr, bit for bit, a NaN's payload included on the device and in numpy alike)"""
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    q = q_of(states["thr"], q_min, q_max)
    applies = states["depth"] >= first_depth
    u = draw(states["seed"], states["pixel"], states["sample"], np.maximum(states["depth"], 1))
    keep = ~applies | (u < q)
    scale = np.where(applies, f32(1.0) / q, f32(1.0)).astype(f32)
    return keep.astype(np.uint8), scale


def apply(items, first_depth, q_min, q_max):
    """a copy of SHADED_DTYPE records after the rule: what roulette_count_kernel leaves in the buffer it counts"""
    out = np.array(items, copy=True)
    go = np.flatnonzero((out["status"] == ffi.VK_SHADE_SCATTERED) & (out["state"]["depth"] >= first_depth))
    keep, scale = rule(out["state"][go], first_depth, q_min, q_max)
    kept, gone = go[keep != 0], go[keep == 0]
    state = out["state"]
    thr = state["thr"]
    with np.errstate(invalid="ignore", over="ignore"):        # (the records' other throughputs are random bits)
        thr[kept] = (thr[kept] * scale[keep != 0, None]).astype(f32)
    out["status"][gone] = ffi.VK_PATHS_CULLED
    return out


# ---- the edge throughputs: name -> (thr, the q the rule must find for q_min, q_max), as a function of the two bounds
def edge_throughputs(q_min, q_max):
    nan, inf = f32(np.nan), f32(np.inf)
    lo, hi = f32(q_min), f32(q_max)
    mid = f32((float(lo) + float(hi)) / 2)
    den = np.uint32(0x00000123).view(f32)          # a denormal
    cases = {
        "nan_in_one": ((nan, mid, f32(0.0)), mid),
        "nan_first_and_last": ((nan, f32(-1.0), nan), lo),
        "nan_in_all": ((nan, nan, nan), lo),
        "plus_inf": ((f32(0.5), inf, f32(0.25)), hi),
        "minus_inf": ((-inf, -inf, -inf), lo),
        "zero": ((f32(0.0), f32(0.0), f32(0.0)), lo),
        "minus_zero": ((f32(-0.0), f32(-0.0), f32(-0.0)), lo),
        "negative": ((f32(-3.0), f32(-0.5), f32(-1e-9)), lo),
        "denormal": ((den, f32(0.0), den), lo),
        "max_at_q_min": ((lo, f32(0.0), np.nextafter(lo, f32(0.0))), lo),
        "max_at_q_max": ((np.nextafter(hi, f32(0.0)), hi, f32(0.0)), hi),
        "just_above_q_min": ((np.nextafter(lo, f32(2.0)), f32(0.0), f32(0.0)), np.nextafter(lo, f32(2.0)) if lo < hi else hi),
        "above_q_max": ((f32(7.5), f32(0.1), f32(0.2)), hi),
        "inside": ((f32(0.0), f32(0.0), mid), mid),
    }
    names = list(cases)
    thr = np.array([cases[k][0] for k in names], f32)
    q = np.array([cases[k][1] for k in names], f32)
    return names, thr, q


def edge_items(status, first_depth, q_min, q_max, seed=0):
    """(items, ids, n_ids): paths_ref.items_for's records — random bytes everywhere —, every second one given an edge throughput, and
    depths first_depth - 1, first_depth, first_depth + 1 and a deep one in turn on all but every seventh, whose random depth stays"""
    import paths_ref
    items, ids, n_ids = paths_ref.items_for(status, seed)
    n = len(items)
    _, thr, _ = edge_throughputs(q_min, q_max)
    state = items["state"]
    i = np.arange(n)
    t = state["thr"]
    t[::2] = thr[(i[::2] // 2) % len(thr)]
    d = state["depth"]
    d[:] = np.where(i % 7 == 3, d, np.asarray([first_depth - 1, first_depth, first_depth + 1, 49], np.uint32)[i % 4])
    return items, ids, n_ids


# ---- the unbiasedness statistic
def channel_z(acc_a, acc_b):
    """per channel: |mean_a - mean_b| / sqrt(se_a^2 + se_b^2), over the finite-filtered acc (a sample with a non-finite component counts
    as zero, as the film counts it), the standard errors from the sample variances"""
    out = []
    stats = []
    for acc in (acc_a, acc_b):
        a = np.asarray(acc, np.float64).reshape(-1, 3).copy()
        a[~np.isfinite(a).all(axis=1)] = 0.0
        stats.append((a.mean(axis=0), a.var(axis=0, ddof=1) / len(a)))
    (ma, va), (mb, vb) = stats
    for c in range(3):
        out.append(float(abs(ma[c] - mb[c]) / np.sqrt(va[c] + vb[c])))
    return out
