"""Randomised material and texture graphs on fixed, simple geometry: the counterpart of test_fuzz_scenes.Gen, which randomises geometry
over eight fixed materials.  MatGen(seed).build() returns (desc, cam, params) like Gen.

The room of special_scenes._room, seen from its open side, holds a 4 x 4 array of carriers facing the camera, one material each: six
spheres that are direct children of the BVH (the device's plain-sphere paths and cooperative_turb see them), a moving sphere, a rect, a
Boxy, a generic list, a sphere under Translate + Rotate, and five media (boundaries: sphere, Boxy, rect, moving sphere, generic list)
whose phase functions are Isotropic over solid, image, checker and noise textures.

What varies is drawn from the lists below.  Which entry a scene takes is decided by rotating counters over the scene's ordinal, so that
a short run of consecutive seeds meets every entry (tests/test_material_graphs.py asserts it from the oracle's first hits); colours,
texels, Perlin tables, the shape of a nested graph and the side a chain hangs on come from the seeded generator.

The seed decides the kind of scene (KIND_OF_SEED): 'pdf' (the HEAD integrator, SpecDiffuse, a light list of 1 to 5 entries of every
kind), 'scatter' (the scatter integrator under the sky: no SpecDiffuse, which has no Material::scatter), and 'plain_pdf' /
'plain_scatter': solid textures only, no SpecDiffuse, no moving sphere and no medium, so that the scene stays on the kernel instance
of Cornell-type scenes while its Metals and Dielectrics take the extreme parameters.

Every carrier records, in `tags`, what its material graph contains; `self.carriers` is a list of (name, material index, tags).  A
medium bounded by a rect is never hit: ConstantMedium::hit asks its boundary twice (hittable.rs:457-458) and a rect answers once.  It
is built all the same (the boundary walk runs), carries the tag ('boundary', 'rect') and is the one carrier in `never_hit`."""
import numpy as np

import special_scenes
from descs import Desc, camera, params
from vecchio_amd import ffi

L, M, D, E, I, S = (ffi.VK_MAT_LAMBERTIAN, ffi.VK_MAT_METAL, ffi.VK_MAT_DIELECTRIC, ffi.VK_MAT_DIFFUSE_LIGHT, ffi.VK_MAT_ISOTROPIC,
                    ffi.VK_MAT_SPEC_DIFFUSE)
KINDS = (L, M, D, E, I, S)
TEX_KINDS = ("solid", "image", "checker", "noise")
TEXTURED = (L, M, E, I)
IMAGE_SIZES = ((1, 1), (1, 7), (7, 1), (5, 3), (8, 8), (32, 16))         # width x height
NOISE_SCALES = (0.0, 0.7, 4.0, -3.0)
FUZZ = (0.0, 0.3, 1.0, 2.5)
REF_IDX = (1.5, 1.0, 0.7, 2.4)
PCT = (0.0, 0.5, 1.0, -0.5, 1.5)
D_TEX, D_MAT = ffi.VK_MAX_CHECKER_DEPTH, ffi.VK_MAX_SPEC_DIFFUSE_DEPTH     # deepest chains the kernel resolves
CHECKER_DEPTHS = (1, 2, 3, D_TEX)
SD_CHAINS = ((1, "spec"),) + tuple((n, side) for n in (2, 3, D_MAT) for side in ("spec", "diffuse", "mixed"))
SD_PAIRS = tuple((a, b) for a in KINDS for b in KINDS)
LIGHT_KINDS = ("rect", "flipped_rect", "sphere", "negative_sphere", "boxy", "list", "moving_sphere", "medium", "translate", "duplicate")
BOUNDARIES = ("sphere", "boxy", "rect", "moving_sphere", "list")
MAX_DEPTHS = (2, 8, 50)
N_SEEDS = 40


def kind_of_seed(seed):
    r = seed % 10
    return "plain_pdf" if r == 4 else "plain_scatter" if r == 9 else "scatter" if r in (1, 6) else "pdf"


def ordinal(seed):
    """the scene's number among the scenes of its own kind"""
    return sum(kind_of_seed(s) == kind_of_seed(seed) for s in range(seed))


class MatGen:
    def __init__(self, seed):
        self.seed = seed
        self.kind = kind_of_seed(seed)
        self.k = ordinal(seed)
        self.plain = self.kind.startswith("plain")
        self.use_pdf = self.kind in ("pdf", "plain_pdf")
        self.r = np.random.default_rng(7000 + seed)
        self.d = Desc()
        self.carriers, self.never_hit, self.light_kinds = [], set(), []
        self.n = dict(pct=self.k, fuzz=self.k, ior=self.k, tex=self.k, scale=self.k, leaf=self.k)

    def turn(self, name, items):
        """the next entry of `items` by the rotating counter `name`"""
        v = items[self.n[name] % len(items)]
        self.n[name] += 1
        return v

    # ------------------------------------------------------------ textures
    def colour(self, lo=0.15, hi=0.95):
        return tuple(float(x) for x in self.r.uniform(lo, hi, 3))

    def make_textures(self):
        d, k = self.d, self.k
        self.images, self.noises, self.checkers = {}, [], {}
        if self.plain:                  # (a texture record that is not solid moves the scene to the everything-instance, used or not)
            return
        for size in (IMAGE_SIZES[k % 6], IMAGE_SIZES[(k + 3) % 6]):
            self.images[size] = d.image(self.r.integers(0, 256, (size[1], size[0], 3)))
        self.noises = [d.noise(self.turn("scale", NOISE_SCALES), seed=2 * self.seed + j) for j in range(2)]
        for depth in sorted((CHECKER_DEPTHS[k % 4], CHECKER_DEPTHS[(k + 1) % 4])):
            self.checkers[depth] = self.checker_chain(depth)

    def shallow(self, tags, max_checker_depth=0):
        """a solid, an image, a noise texture, or one of the checkers built so far that is at most max_checker_depth deep"""
        fit = [n for n in self.checkers if n <= max_checker_depth]
        c = int(self.r.integers(0, 4 if fit else 3))
        if c == 0:
            return self.d.solid(*self.colour())
        if c == 1:
            size = list(self.images)[int(self.r.integers(0, len(self.images)))]
            tags.add(("image", size))
            return self.images[size]
        if c == 2:
            return self.noises[int(self.r.integers(0, 2))]
        t, ctags = self.checkers[fit[int(self.r.integers(0, len(fit)))]]
        tags |= ctags
        return t

    def checker_chain(self, depth):
        """(texture, tags): `depth` checkers on the longest path.  A point takes the same side at every level (the sign of the sines
        depends on the point alone), so the chain hangs on one side throughout — half of all points walk all of it — and now and then
        on both; the other child is a texture of any kind, an earlier checker that does not make the path longer included."""
        tags = {("checker_depth", depth)}
        side = int(self.r.integers(0, 2))
        t = self.shallow(tags)
        for level in range(depth):
            other = t if (level > 0 and self.r.uniform() < 0.25) else self.shallow(tags, max_checker_depth=level)
            t = self.d.checker(t, other) if side == 0 else self.d.checker(other, t)
        return t, tags

    def texture(self, kind, tags, bright=False):
        if self.plain:
            kind = "solid"
        if kind == "solid":
            return self.d.solid(*(self.colour(2.0, 9.0) if bright else self.colour()))
        if kind == "image":
            size = list(self.images)[self.n["tex"] % 2]
            tags.add(("image", size))
            return self.images[size]
        if kind == "noise":
            return self.noises[self.n["tex"] % 2]
        depth = list(self.checkers)[self.n["tex"] % 2]
        t, ctags = self.checkers[depth]
        tags |= ctags
        return t

    # ------------------------------------------------------------ materials
    def leaf(self, kind, tags, tex_kind=None):
        d = self.d
        if kind == D:
            ior = self.turn("ior", REF_IDX)
            tags.add(("ref_idx", ior))
            return d.mat(D, 0, ior)
        tex_kind = tex_kind or self.turn("tex", TEX_KINDS)
        if self.plain:
            tex_kind = "solid"
        tags.add(("mat_tex", kind, tex_kind))
        tex = self.texture(tex_kind, tags, bright=kind == E and tex_kind == "solid")     # textured lights emit at most 1
        param = 0.0
        if kind == M:
            param = self.turn("fuzz", FUZZ)
            tags.add(("fuzz", param))
        return d.mat(kind, tex, param)

    def any_leaf(self, tags):
        return self.leaf(self.turn("leaf", (L, M, D, E, I)), tags)

    def spec_diffuse(self, a, b, tags):
        pct = self.turn("pct", PCT)
        tags.add(("pct", pct))
        return self.d.mat(S, 0, pct, a, b)

    def child(self, kind, tags):
        if kind == S:
            return self.spec_diffuse(self.any_leaf(tags), self.any_leaf(tags), tags)
        return self.leaf(kind, tags)

    def sd_pair(self, ks, kd):
        tags = {("sd_pair", ks, kd), ("sd_depth", 2 if S in (ks, kd) else 1)}
        return self.spec_diffuse(self.child(ks, tags), self.child(kd, tags), tags), tags

    def sd_chain(self, depth, side):
        tags = {("sd_depth", depth), ("sd_chain", depth, side)}
        m = self.spec_diffuse(self.any_leaf(tags), self.any_leaf(tags), tags)
        for level in range(1, depth):
            on_spec = side == "spec" or (side == "mixed" and level % 2 == 1)
            other = self.any_leaf(tags)
            m = self.spec_diffuse(m, other, tags) if on_spec else self.spec_diffuse(other, m, tags)
        return m, tags

    def surface_materials(self, n):
        """n (material, tags) for the surface carriers"""
        out = []
        if self.kind == "pdf":
            for t in range(4):
                out.append(self.sd_pair(*SD_PAIRS[(4 * self.k + t) % len(SD_PAIRS)]))
            out.append(self.sd_chain(*SD_CHAINS[self.k % len(SD_CHAINS)]))
        # the rest: Lambertian / Metal / DiffuseLight over every texture kind and Dielectric, six and more a scene
        table = [(kind, tex) for kind in (L, M, E) for tex in TEX_KINDS] + [(D, None)] * 4
        start = self.k * (n - len(out))
        for j in range(n - len(out)):
            kind, tex = table[(start + j) % len(table)]
            tags = set()
            out.append((self.leaf(kind, tags, tex), tags))
        order = self.r.permutation(n)           # which carrier takes which
        return [out[i] for i in order]

    # ------------------------------------------------------------ geometry
    @staticmethod
    def slot(i):
        return np.array([1.4 + 2.4 * (i % 4), 1.3 + 2.4 * (i // 4), 4.5])

    def carrier(self, name, ref, mat, tags):
        self.carriers.append((name, mat, tags))
        self.refs.append(ref)

    def build(self):
        d = self.d
        lights = []
        self.refs = special_scenes._room(d, lights)
        wall = 0                                                       # the room's white Lambertian: what a boundary is made of
        self.make_textures()
        n_surface = 16 if self.plain else 11
        mats = self.surface_materials(n_surface)
        R = 0.85
        slot = 0
        spheres = []
        for _ in range(6 if not self.plain else 12):
            m, tags = mats[slot]
            ref = d.sphere(tuple(self.slot(slot)), R, m)
            self.carrier("sphere", ref, m, tags); spheres.append(ref); slot += 1
        moving = None
        if not self.plain:
            m, tags = mats[slot]; c = self.slot(slot)
            moving = d.moving_sphere(tuple(c), tuple(c + (0.3, 0.1, 0.0)), 0.0, 1.0, 0.75, m)
            self.carrier("moving_sphere", moving, m, tags); slot += 1
        # rect: its corners are in view, so u and v run over all of [0, 1]; facing the camera or away from it by the ordinal
        m, tags = mats[slot]; c = self.slot(slot)
        ref = d.xy_rect(c[0] - R, c[0] + R, c[1] - R, c[1] + R, 4.5, m)
        self.carrier("rect", Desc.flip(ref) if self.k % 2 else ref, m, tags); slot += 1
        m, tags = mats[slot]; c = self.slot(slot)
        self.carrier("boxy", d.boxy(tuple(c - 0.7), tuple(c + 0.7), m), m, tags); slot += 1
        m, tags = mats[slot]; c = self.slot(slot)
        self.carrier("list", d.list_([d.sphere(tuple(c), 0.7, m), d.xy_rect(c[0] - R, c[0] + R, c[1] - R, c[1] + R, 5.5, m)]), m, tags); slot += 1
        m, tags = mats[slot]; c = self.slot(slot)
        self.carrier("transformed_sphere", d.translate(d.rotate(d.sphere((0, 0, 0), R, m), int(self.k % 3), 35.0), tuple(c)), m, tags); slot += 1
        media = []
        if not self.plain:
            for bk in BOUNDARIES:
                c = self.slot(slot)
                if bk == "sphere":
                    b = d.sphere(tuple(c), 0.95, wall)
                elif bk == "boxy":
                    b = d.boxy(tuple(c - 0.8), tuple(c + 0.8), wall)
                elif bk == "rect":
                    b = d.xy_rect(c[0] - R, c[0] + R, c[1] - R, c[1] + R, 4.5, wall)
                elif bk == "moving_sphere":
                    b = d.moving_sphere(tuple(c), tuple(c + (0.25, 0.0, 0.0)), 0.0, 1.0, 0.9, wall)
                else:
                    b = d.list_([d.sphere(tuple(c), 0.95, wall), d.xy_rect(c[0] - 0.2, c[0] + 0.2, c[1] - 0.2, c[1] + 0.2, 9.0, wall)])
                tags = {("boundary", bk)}
                iso = self.leaf(I, tags, TEX_KINDS[(self.k + slot) % 4])
                ref = d.medium(b, float(self.r.uniform(1.5, 4.0)), iso)
                self.carrier("medium_" + bk, ref, iso, tags); media.append(ref); slot += 1
                if bk == "rect":
                    self.never_hit.add(iso)
        assert slot == 16
        if self.use_pdf:
            lights = self.make_lights(lights[0], moving, media)
        world = special_scenes._bvh_chain(d, self.refs)
        desc = d.finish(world, lights if self.use_pdf else [])
        cam = camera((5, 5, -12), (5, 5, 0), vfov=40.0)
        depth = MAX_DEPTHS[self.k % 3]
        if self.use_pdf:
            p = params(24, 24, 4, max_depth=depth, seed=100 + self.seed)
        else:
            p = params(24, 24, 4, max_depth=depth, seed=100 + self.seed, integrator=ffi.VK_INTEGRATOR_SCATTER,
                       background=ffi.VK_BACKGROUND_SKY)
        return desc, cam, p

    def make_lights(self, ceiling, moving, media):
        """1 to 5 entries; ten consecutive ordinals meet every kind.  Emitters the list names are put into the world, below the
        ceiling and behind the carriers; a moving sphere, a medium and a Translate have the trait's defaults (pdf 0, direction
        (1, 0, 0)), whatever they are made of."""
        d, k = self.d, self.k
        emit = d.light(*self.colour(3.0, 9.0))
        start, n = (3 * k) % 10, (5, 3, 1, 4, 2)[k % 5]
        out = []
        for j in range(n):
            kind = LIGHT_KINDS[(start + j) % 10]
            x = 1.0 + 0.85 * ((start + j) % 10)
            if kind in ("moving_sphere", "medium") and self.plain:
                kind = "rect"                                          # (a plain scene has neither)
            if kind == "rect":
                ref = ceiling
            elif kind == "flipped_rect":
                ref = Desc.flip(ceiling)
            elif kind in ("sphere", "negative_sphere"):
                ref = d.sphere((x, 8.8, 8.5), 0.35 if kind == "sphere" else -0.35, emit); self.refs.append(ref)
            elif kind == "boxy":
                ref = d.boxy((x - 0.3, 8.5, 8.2), (x + 0.3, 9.1, 8.8), emit); self.refs.append(ref)
            elif kind == "list":
                ref = d.list_([d.xz_rect(x - 0.3, x + 0.3, 8.0, 8.6, 9.3, emit), d.xy_rect(x - 0.3, x + 0.3, 8.4, 9.0, 9.2, emit)])
                self.refs.append(ref)
            elif kind == "moving_sphere":
                ref = moving
            elif kind == "medium":
                ref = media[k % len(media)]
            elif kind == "translate":
                ref = d.translate(d.sphere((0, 0, 0), 0.3, emit), (x, 8.8, 8.5)); self.refs.append(ref)
            else:                                                      # the entry before it once more (the ceiling when there is none)
                if not out:
                    out.append(ceiling); self.light_kinds.append("rect")
                ref = out[-1]
            out.append(ref); self.light_kinds.append(kind)
        return out


_CACHE = {}


def scene(seed):
    """(generator, desc, cam, params) of MatGen(seed), built once (the generator owns the arrays the description points into)"""
    if seed not in _CACHE:
        g = MatGen(seed)
        _CACHE[seed] = (g,) + tuple(g.build())
    return _CACHE[seed]


def hits_per_material(oracle, desc, cam, p):
    """primary samples whose first hit has material i, from the oracle's first hits"""
    fh = oracle.first_hits(desc, cam, p, 0, p.samples_per_pixel)
    hit = fh["hit"] != 0
    return np.bincount(fh["material"][hit].astype(np.int64), minlength=desc.contents.n_materials)


def required_tags():
    """everything that must occur on a carrier that is hit, over a set of seeds"""
    want = {("mat_tex", kind, tex) for kind in TEXTURED for tex in TEX_KINDS}
    want |= {("sd_pair", a, b) for a, b in SD_PAIRS}
    want |= {("pct", v) for v in PCT} | {("fuzz", v) for v in FUZZ} | {("ref_idx", v) for v in REF_IDX}
    want |= {("checker_depth", n) for n in CHECKER_DEPTHS} | {("sd_depth", n) for n in (1, 2, 3, D_MAT)}
    want |= {("sd_chain",) + c for c in SD_CHAINS}
    want |= {("image", s) for s in IMAGE_SIZES} | {("boundary", b) for b in BOUNDARIES if b != "rect"}
    return want


def coverage(oracle, seeds, min_hits=8):
    """(tags seen on carriers hit by >= min_hits primary samples, light kinds seen, boundary kinds built) over `seeds`; asserts that
    every carrier of every scene is hit, but for the rect-bounded medium, which must never be"""
    seen, light_kinds, boundaries = set(), set(), set()
    for seed in seeds:
        g, desc, cam, p = scene(seed)
        n = hits_per_material(oracle, desc, cam, p)
        for name, mat, tags in g.carriers:
            if mat in g.never_hit:
                assert n[mat] == 0, f"seed {seed}: the rect-bounded medium was hit"
                boundaries.add("rect")
                continue
            assert n[mat] >= min_hits, f"seed {seed}: carrier {name} (material {mat}) has {int(n[mat])} primary hits"
            seen |= tags
        light_kinds |= set(g.light_kinds)
        boundaries |= {t[1] for _, _, tags in g.carriers for t in tags if t[0] == "boundary"}
    return seen, light_kinds, boundaries


# ---------------------------------------------------------------- chains at and beyond the limits (tests/test_validation.py)
def _one_ball(d, refs, lights, m):
    refs.append(d.sphere((5, 4, 5), 3.0, m))
    world = special_scenes._bvh_chain(d, refs)
    return d, d.finish(world, lights), camera((5, 5, -12), (5, 5, 0), vfov=40.0), params(24, 24, 4, max_depth=8, seed=3)


def checker_chain_scene(depth):
    """a ball in the room whose Lambertian reads `depth` nested checkers, each with the next one as BOTH children (whatever the sign
    of the sines, every point walks the whole chain), above a checker of two solids"""
    d = Desc()
    lights = []
    refs = special_scenes._room(d, lights)
    t = d.checker(d.solid(0.9, 0.2, 0.1), d.solid(0.1, 0.9, 0.8))
    for _ in range(depth - 1):
        t = d.checker(t, t)
    return _one_ball(d, refs, lights, d.mat(L, t))


def spec_diffuse_chain_scene(depth, side):
    """a ball in the room under `depth` nested SpecDiffuses, the chain on the 'spec', the 'diffuse' or on alternating ('mixed') sides"""
    d = Desc()
    lights = []
    refs = special_scenes._room(d, lights)
    m = d.lambertian(0.8, 0.3, 0.2)
    for level in range(depth):
        on_spec = side == "spec" or (side == "mixed" and level % 2 == 1)
        if on_spec:
            m = d.mat(S, 0, 0.5, m, d.lambertian(0.2, 0.3, 0.9))
        else:
            m = d.mat(S, 0, 0.5, d.mat(M, d.solid(0.9, 0.9, 0.7), 0.3), m)
    return _one_ball(d, refs, lights, m)


def image_edge_scene(size=(5, 3)):
    """an image-textured rect far from the origin, where the f32 grid is coarse (1/32 at 2^18) against the rect's half unit: one hit
    point in some tens lies exactly on the rect's far edge, where u (or v) is exactly 1 and u * width is the index one past the row —
    the texel clamp of ImageTexture::value (material.rs:283-303) decides the colour of those samples"""
    d = Desc()
    rng = np.random.default_rng(17)
    tex = d.image(rng.integers(0, 256, (size[1], size[0], 3)))
    far = 262144.0
    r = d.xy_rect(far, far + 0.5, far, far + 0.5, 8.0, d.mat(L, tex))
    desc = d.finish(d.big_box(r, r))
    cam = camera((far + 0.25, far + 0.25, 6.0), (far + 0.25, far + 0.25, 8.0), vfov=20.0)
    return d, desc, cam, params(24, 24, 4, max_depth=2, seed=9, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)
