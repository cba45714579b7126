"""Light-path layers on the CPU: the kernels' own per-lane code (vk_lpe.h, built with g++ into tests/emu) against tests/lpe_ref.py's numpy
restatement of the header's definition — the event code, the tag update (exhaustively over status, lobe and bounce number), the rule
match and the resolve on random rules, tags and cells.  Then the tags of emulated camera-path batches on the three scenes the device
test uses: which nibbles are set, what the last one says, how state.depth follows the bounces, what a path that ended on a light
carries — and that every scene has paths of more than seven bounces, which the device test relies on."""
import numpy as np
import pytest

import emu_lpe_ffi as EMU
import lpe_ref as L
from vecchio_amd import ffi
from vecchio_amd.scene import standard_rules, STANDARD_LAYERS

u32 = np.uint32
f32 = np.float32
STATUSES = range(6)
LOBES = list(range(9)) + [0xFFFFFFFF]
BOUNCES = range(10)


def test_event_code_and_tag_update_exhaustively(emu):
    status, lobe = (a.reshape(-1) for a in np.meshgrid(np.array(STATUSES, u32), np.array(LOBES, u32), indexing="ij"))
    code = L.event_code(status, lobe)
    assert np.array_equal(EMU.event_codes(status, lobe), code)
    # the table of the header, spelled out
    for s, l, c in zip(status.tolist(), lobe.tolist(), code.tolist()):
        want = 1 if s == ffi.VK_SHADE_MISS else 15 if s == ffi.VK_SHADE_BAD_HIT else 2 + l if l <= 5 else 14
        assert c == want, (s, l)
    assert set(code.tolist()) == {1, 2, 3, 4, 5, 6, 7, 14, 15}
    rng = np.random.default_rng(3)
    n = len(status)
    ids = rng.permutation(n + 5)[:n].astype(u32)             # every id at most once, some ids of the table never
    for b in BOUNCES:
        sig0, term0 = rng.integers(0, 1 << 32, n + 5, dtype=np.uint64).astype(u32), rng.integers(0, 1 << 32, n + 5, dtype=np.uint64).astype(u32)
        hit, material = rng.integers(0, 3, n).astype(u32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u32)
        got_sig, got_term = sig0.copy(), term0.copy()
        EMU.record(got_sig, got_term, b, ids, status, lobe, hit, material)
        want_sig, want_term = sig0.copy(), term0.copy()
        shaded = np.zeros(n, [("status", u32), ("lobe", u32)])
        shaded["status"], shaded["lobe"] = status, lobe
        hits = np.zeros(n, [("hit", u32), ("material", u32)])
        hits["hit"], hits["material"] = hit, material
        L.record(want_sig, want_term, b, ids, hits, shaded)
        assert np.array_equal(got_sig, want_sig) and np.array_equal(got_term, want_term), b
        # spelled out: nibble b (b < 7) and nibble 7 are the code, every other nibble is what it was — all zero behind bounce 0
        for j in range(n):
            s, c, old = int(got_sig[ids[j]]), int(code[j]), int(sig0[ids[j]])
            assert s >> 28 == c and (b >= 7 or (s >> 4 * b) & 0xF == c)
            keep = 0x0FFFFFFF & ~(0xF << 4 * b if b < 7 else 0)
            assert s & keep == (old & keep if b else 0), (b, j)
            assert int(got_term[ids[j]]) == (int(material[j]) if hit[j] == 1 else 0xFFFFFFFF)
        untouched = np.setdiff1d(np.arange(n + 5), ids)
        assert np.array_equal(got_sig[untouched], sig0[untouched]) and np.array_equal(got_term[untouched], term0[untouched])


def random_rules(rng, n_rules, n_layers):
    rules = []
    for _ in range(n_rules):
        mask = 0
        for b in rng.choice(8, int(rng.integers(0, 3)), replace=False):
            mask |= 0xF << (4 * int(b))
        value = int(rng.integers(0, 1 << 32)) & mask if rng.random() < 0.8 else (int(rng.integers(1, 8)) * 0x11111111) & mask
        smask = int(rng.choice([1, 4, 16, 5, 20, 17, 21]))
        d0 = int(rng.integers(0, 6))
        d1 = d0 + int(rng.integers(0, 6)) if rng.random() < 0.8 else 0xFFFFFFFF
        emitter = 0xFFFFFFFF if rng.random() < 0.7 else int(rng.integers(0, 4))
        rules.append(ffi.LpeRule(mask, value, smask, d0, d1, emitter, int(rng.integers(0, n_layers)), 0))
    return rules


def test_rule_match_on_random_rules_and_tags(emu):
    rng = np.random.default_rng(11)
    n = 4000
    hit_layers, matched = set(), 0
    for trial in range(40):
        n_layers = int(rng.integers(1, 17))
        rules = random_rules(rng, int(rng.integers(0, 33)), n_layers)
        rest = int(rng.integers(0, n_layers))
        status = rng.choice([ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED, ffi.VK_PATHS_CULLED], n).astype(u32)
        depth = rng.integers(0, 12, n).astype(u32)
        # tags made of small codes, so that masks of one or two nibbles do match
        sig = np.zeros(n, np.uint64)
        for b in range(8):
            sig |= rng.integers(0, 8, n).astype(np.uint64) << np.uint64(4 * b)
        term = np.where(rng.random(n) < 0.3, 0xFFFFFFFF, rng.integers(0, 4, n)).astype(u32)
        want = L.layers_of(rules, rest, status, depth, sig.astype(u32), term)
        got = EMU.layers_of(rules, rest, status, depth, sig.astype(u32), term)
        assert np.array_equal(got, want), trial
        assert (want < n_layers).all()
        # first match wins: spelled out for a few results
        for i in range(0, n, 401):
            first = next((r.layer for r in rules if (int(sig[i]) & r.sig_mask) == r.sig_value and (r.status_mask >> int(status[i])) & 1 and
                          r.depth_min <= depth[i] <= r.depth_max and r.emitter in (0xFFFFFFFF, int(term[i]))), rest)
            assert want[i] == first
        hit_layers |= set(want.tolist())
        matched += int((want != rest).sum())
    assert len(hit_layers) == 16 and matched > 40 * n // 4


def test_resolve_of_cells(emu):
    rng = np.random.default_rng(5)
    cells = rng.integers(-(1 << 40), 1 << 40, (500, 4))
    cells[:50] = rng.integers(-(1 << 62), 1 << 62, (50, 4))
    cells[50:60] = 0
    cells[:, 3] = rng.integers(0, 1 << 20, 500)
    for n in (1, 3, 12, 1 << 20, 0xFFFFFFFF):
        rgb, share = EMU.resolve(cells, n)
        state = cells.reshape(500, 1, 4)
        want_rgb, want_share = L.resolve(state, 0, n)
        assert np.array_equal(rgb.view(u32), want_rgb.view(u32)) and np.array_equal(share.view(u32), want_share.view(u32)), n
    # VK_LPE_ALL adds the integers first: three layers whose f32 images would not add up to it
    state = np.zeros((1, 3, 4), np.int64)
    state[0, :, 0] = (1 << 26) + 1, (1 << 50), -(1 << 50)
    state[0, :, 3] = 1, 2, 3
    rgb, share = L.resolve(state, L.ALL, 2)
    assert rgb[0, 0] == f32(((1 << 26) + 1) * 2.0 ** -26) / f32(2) and share[0] == 3.0
    assert np.array_equal(EMU.resolve(state.sum(axis=1), 2)[0].view(u32), rgb.view(u32))


# ---------------------------------------------------------------- tags of emulated batches
def nibbles(sig):
    return (np.asarray(sig, np.int64)[:, None] >> (4 * np.arange(8))) & 0xF


@pytest.mark.parametrize("kind,name,integrator", L.SCENES, ids=[s[1] for s in L.SCENES])
def test_tags_of_emulated_batches(kind, name, integrator, emu, host_scenes):
    desc, cam, p = L.scene(kind, name, host_scenes)
    d = desc.contents
    deep = 0
    for W, H in L.FRAMES:
        q = L.frame_params(p, W, H, integrator)
        assert q.max_depth == 12
        states, status, sig, term, taken = L.emulated_frame(desc, cam, q, name)
        nib = nibbles(sig)
        assert (taken >= 1).all() and taken.max() <= 13
        for k in range(1, 8):
            sel = taken == k
            assert (nib[sel, :k] != 0).all() and (nib[sel, k:7] == 0).all() and (nib[sel, 7] == nib[sel, k - 1]).all(), (name, k)
        sel = taken > 7
        assert (nib[sel] != 0).all()
        deep += int(sel.sum())
        # state.depth against the bounces taken.  A bounce adds 1 to the depth where the path scatters: not on a miss, not on a light
        # and not on an absorbing Metal, which end the path before the depth moves.  So a path of k bounces has depth k — a rule that
        # wants "light met on segment k" asks for depth k — but for the path the depth limit ended: its last bounce did scatter, it
        # has depth k + 1 = max_depth + 1, and "depth - 1 = bounces taken" holds for it alone.
        assert set(status.tolist()) <= {ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED}
        left = status == ffi.VK_SHADE_MISS
        on_light = (status == ffi.VK_SHADE_ENDED) & (nib[:, 7] == ffi.VK_LPE_EMIT)
        cut = states["depth"] > q.max_depth
        assert np.array_equal(states["depth"].astype(np.int64), taken + cut), name
        assert cut.any() and (states["depth"][cut] - 1 == taken[cut]).all() and (taken[cut] == q.max_depth).all()
        assert not (cut & (left | on_light)).any()
        assert ((nib[:, 7] == ffi.VK_LPE_SKY) == left).all() and ((term == 0xFFFFFFFF) == left).all()
        # a path that ended on a DiffuseLight: last code 5, term a DiffuseLight material
        lit = nib[:, 7] == ffi.VK_LPE_EMIT
        assert (status[lit] == ffi.VK_SHADE_ENDED).all()
        kinds = np.array([d.materials[i].kind for i in range(d.n_materials)])
        assert (term[~left] < d.n_materials).all()
        assert (kinds[term[lit]] == ffi.VK_MAT_DIFFUSE_LIGHT).all()
        ended_elsewhere = (status == ffi.VK_SHADE_ENDED) & ~lit
        assert (kinds[term[ended_elsewhere]] != ffi.VK_MAT_DIFFUSE_LIGHT).all()
        if name != "scatter_sky":
            assert lit.any(), name
        # the standard rules put every path with light on it somewhere else than "rest", and nothing lit is in "rest"
        layer = L.layers_of(standard_rules(), STANDARD_LAYERS.index("rest"), status, states["depth"], sig, term)
        carries = lit | left
        assert (layer[carries] != STANDARD_LAYERS.index("rest")).all() and (layer[~carries & (nib[:, 0] != 6)] == STANDARD_LAYERS.index("rest")).all()
    assert deep >= 1, f"{name}: no path of more than 7 bounces at max_depth 12 (tests/test_gpu_lpe.py relies on one)"
