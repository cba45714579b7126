"""vk_lpe_* restated in numpy from the definition in include/vecchio_amd.h ("light-path layers"): a bounce's event code, the update of a
path's tag, the match of a result against the rules, the deposit (tests/film_ref.py's conversion, on top of tests/exact_sums.py) and the
resolve of a layer.  What tests/test_lpe_emu.py and tests/test_gpu_lpe.py share."""
import numpy as np

import exact_sums as E
import film_ref as F
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32
u32 = np.uint32
COUNTERS = ("deposited", "dropped", "clamped", "skipped")
INV_SCALE = f32(2.0 ** -26)
ALL = ffi.VK_LPE_ALL
NO_TERM = 0xFFFFFFFF


def event_code(status, lobe):
    """the 4-bit code of a bounce's record: MISS 1, BAD_HIT 15, else 2 + lobe for lobe 0..5 and 14 for any other lobe"""
    status, lobe = np.asarray(status, np.int64), np.asarray(lobe, np.int64)
    by_lobe = np.where((lobe >= 0) & (lobe <= 5), 2 + lobe, ffi.VK_LPE_OTHER)
    return np.where(status == ffi.VK_SHADE_MISS, ffi.VK_LPE_SKY, np.where(status == ffi.VK_SHADE_BAD_HIT, ffi.VK_LPE_BAD, by_lobe)).astype(u32)


def tag_update(sig, bounce, code):
    """the tag's first word after bounce number `bounce` (0 the first) with event `code`"""
    sig, code = np.asarray(sig, np.int64), np.asarray(code, np.int64)
    if bounce == 0:
        return (code | (code << 28)).astype(u32)
    if bounce < 7:
        sig = (sig & ~(0xF << (4 * bounce))) | (code << (4 * bounce))
    return ((sig & 0x0FFFFFFF) | (code << 28)).astype(u32)


def term_of(hit, material):
    return np.where(np.asarray(hit) == 1, np.asarray(material, np.int64), NO_TERM).astype(u32)


def record(sig, term, bounce, ids, hits, shaded):
    """one bounce of a batch on the tables sig, term (uint32 per id, changed in place): ids the bounce's ids in live order, hits and
    shaded its HIT_DTYPE and SHADED_DTYPE records"""
    ids = np.asarray(ids, np.int64)
    sig[ids] = tag_update(sig[ids], bounce, event_code(shaded["status"], shaded["lobe"]))
    term[ids] = term_of(hits["hit"], hits["material"])


def rule_fields(r):
    return {k: int(getattr(r, k)) for k in ("sig_mask", "sig_value", "status_mask", "depth_min", "depth_max", "emitter", "layer")}


def layers_of(rules, rest, status, depth, sig, term):
    """the layer of every result: the first matching rule's, `rest` without one"""
    status, depth = np.asarray(status, np.int64), np.asarray(depth, np.int64)
    sig, term = np.asarray(sig, np.int64), np.asarray(term, np.int64)
    layer = np.full(len(status), rest, np.int64)
    found = np.zeros(len(status), bool)
    for r in rules:
        r = rule_fields(r)
        m = ((sig & r["sig_mask"]) == r["sig_value"]) & (((r["status_mask"] >> np.minimum(status, 31)) & 1) != 0) & \
            (r["depth_min"] <= depth) & (depth <= r["depth_max"]) & ((r["emitter"] == 0xFFFFFFFF) | (r["emitter"] == term))
        m &= ~found
        layer[m] = r["layer"]
        found |= m
    return layer


def deposit(states, status, sig, term, rules, n_layers, rest, width, height, spp, state=None):
    """vk_lpe_deposit in numpy: (state (height, width, n_layers, 4) int64 — added to where given —, dict of the four counters).  The
    film's rule (tests/film_ref.py deposit) with the cell (pixel, layer) and a count that takes the dropped results too."""
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, u32).reshape(-1)
    n_pixels = width * height
    state = np.zeros((height, width, n_layers, 4), np.int64) if state is None else state.copy()
    flat = state.reshape(n_pixels * n_layers, 4)
    ours = np.isin(status, F.DEPOSITING) & (states["pixel"] < n_pixels)
    acc = states["acc"].astype(f32)
    finite = np.isfinite(acc).all(axis=1)
    dep = ours & finite
    clampv = E.accum_clamp_for(spp)
    layer = layers_of(rules, rest, status, states["depth"], sig, term)
    cell = states["pixel"].astype(np.int64) * n_layers + layer
    big = np.abs(acc[dep]).max(axis=1) if dep.any() else np.zeros(0, f32)
    if dep.any():
        add = np.zeros((int(dep.sum()), 4), np.int64)
        add[:, :3] = E.to_fixed(acc[dep], clampv)
        np.add.at(flat, cell[dep], add)
    one = np.zeros((int(ours.sum()), 4), np.int64)
    one[:, 3] = 1
    np.add.at(flat, cell[ours], one)
    counters = dict(deposited=int(dep.sum()), dropped=int((ours & ~finite).sum()),
                    clamped=int(((big > E.ACCUM_SMALL) & (big > clampv)).sum()), skipped=int((~ours).sum()))
    return state, counters


def counters_of(info):
    return {k: int(getattr(info, k)) for k in COUNTERS}


def resolve(state, layer, n):
    """vk_lpe_resolve in numpy: state (..., n_layers, 4) int64 -> (rgb (..., 3) float32, share (...) float32)"""
    state = np.asarray(state, np.int64)
    with np.errstate(over="ignore"):
        cell = state.sum(axis=-2, dtype=np.int64) if layer == ALL else state[..., layer, :]      # (int64 sums wrap as the device's do)
    nf = f32(n)
    rgb = ((cell[..., :3].astype(f32) * INV_SCALE).astype(f32) / nf).astype(f32)
    share = (cell[..., 3].astype(f32) / nf).astype(f32)
    return rgb, share


SPP = 12
FRAMES = [(24, 16), (33, 17)]
SCENES = [("builder", "cornell_box", ffi.VK_INTEGRATOR_PDF), ("special", "media_and_textures", ffi.VK_INTEGRATOR_PDF),
          ("special", "scatter_sky", ffi.VK_INTEGRATOR_SCATTER)]
ROULETTE = (3, 0.1, 0.8)
_FRAMES = {}


def scene(kind, name, host_scenes):
    import shade_ref as S
    return S.scene(kind, name, host_scenes)


def frame_params(p, W, H, integrator, spp=SPP):
    """tests/test_gpu_robust.py's: the scene's parameters at W x H, spp samples, max_depth at most 12"""
    q = ffi.RenderParams.from_buffer_copy(p)
    q.width, q.height, q.samples_per_pixel, q.integrator = W, H, spp, integrator
    q.max_depth = min(int(p.max_depth), 12)
    return q


def emulated_frame(desc, cam, q, name, rule=None):
    """every camera path of the frame on the CPU emulators, computed once per (scene, frame, rule): (states, status, sig, term, bounces
    taken) indexed by pixel * spp + sample (tests/film_ref.py dump_index)"""
    import emu_film_ffi
    import emu_paths_ffi
    import shade_ref as S
    key = (name, q.width, q.height, q.samples_per_pixel, q.integrator, q.max_depth, q.seed, rule)
    if key not in _FRAMES:
        rays, states = emu_film_ffi.emit(cam, q, 0, 0, q.width, q.height, 0, q.samples_per_pixel)
        b = emu_paths_ffi.Batch(desc, **S.shade_kwargs(q, q.integrator, q.max_depth))
        b.begin(rays, states)
        sig, term, taken = emulate(b, len(rays), rule)
        _FRAMES[key] = b.results() + (sig, term, taken)
    return _FRAMES[key]


def emulate(batch, n, rule=None, max_bounces=None, tags=None, first_bounce=0):
    """steps the begun emulated batch (tests/emu_paths_ffi.py Batch) of n paths to its end, or max_bounces bounces: (sig, term, bounces
    taken per id).  rule = (first_depth, q_min, q_max): with the handle's roulette rule, as the compaction's count pass applies it
    (tests/roulette_ref.py apply) — the tags see the records behind it.  tags = (sig, term, taken) of an earlier call and first_bounce
    the bounces the batch has run: the run goes on from there."""
    import emu_paths_ffi
    import emu_shade_ffi
    import roulette_ref
    sig, term, taken = tags if tags is not None else (np.zeros(n, u32), np.zeros(n, u32), np.zeros(n, np.int64))
    b, max_bounces = first_bounce, None if max_bounces is None else first_bounce + max_bounces
    while batch.live and (max_bounces is None or b < max_bounces):
        ids = batch.ids.copy()
        hits, advanced = emu_paths_ffi.trace_paths(batch.desc, batch.rays, batch.states)
        shaded = emu_shade_ffi.shade_hits(batch.desc, batch.rays, hits, advanced, **batch.params)
        if rule is not None:
            shaded = roulette_ref.apply(shaded, *rule)
        batch._compact(shaded)
        record(sig, term, b, ids, hits, shaded)
        taken[ids] += 1
        b += 1
    return sig, term, taken
