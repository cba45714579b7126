"""Randomised material and texture graphs (tests/material_graphs.py) on the CPU: the kernel's shading, texture and first-hit albedo
code (vk_trace.h shade_core, texture_value, aov_albedo, through tests/emu) against the recursive oracle on every sample — SpecDiffuse
over every pair of child kinds and nested to the limit along either side, checkers under checkers to the limit, every material over
every texture kind, images of odd sizes, the extreme Metal / Dielectric / pct parameters, light lists of every kind of entry, media
behind every kind of boundary.  The comparisons are the existing ones, unchanged: test_emu_parity.compare for radiance and draw
counts, test_aov_emu.check_per_sample for the first-hit buffers, test_guides_emu.check_per_sample (bit for bit) for the guides.

That the scenes do contain all of this, on carriers the camera sees, is asserted from the oracle's first hits (material_graphs.coverage)
for the 40 seeds and for the 16 the GPU module runs."""
import pytest

import material_graphs as MG
import test_aov_emu as aov_shared
import test_guides_emu as guides_shared
from test_emu_parity import compare
from test_guides_emu import emu_guides          # noqa: F401  (the fixture)

SEEDS = tuple(range(MG.N_SEEDS))
GPU_SEEDS = tuple(range(16))                     # tests/test_gpu_material_graphs.py
# first-hit albedo: SpecDiffuse chains of depth 2, 3 and D_MAT on the specular, the diffuse and alternating sides, nested checkers
AOV_SEEDS = (2, 3, 7, 8, 10, 12, 13, 15)
GUIDE_SEEDS = (2, 7, 12, 15)


def tags_of(seeds):
    return [tags for seed in seeds for _, _, tags in MG.scene(seed)[0].carriers]


@pytest.mark.parametrize("seed", SEEDS)
def test_material_graph_per_sample(seed, oracle, emu):
    g, desc, cam, p = MG.scene(seed)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    img_e, ps_e, steps, info = emu.render_samples(desc, cam, p)
    compare(ps_o, ps_e, img_o, img_e)
    assert steps > 0
    # the kernel instance the device would run: Cornell-type for the plain scenes, the everything-instance for the others
    assert (info[3] & 0x17F) == (0x116 if g.plain else 0x17F if g.use_pdf else 0x13F)


def check_coverage(oracle, seeds):
    seen, light_kinds, boundaries = MG.coverage(oracle, seeds)
    missing = MG.required_tags() - seen
    assert not missing, f"never on a carrier that is hit: {sorted(missing, key=str)}"
    assert light_kinds == set(MG.LIGHT_KINDS), set(MG.LIGHT_KINDS) - light_kinds
    assert boundaries == set(MG.BOUNDARIES), set(MG.BOUNDARIES) - boundaries
    kinds = {MG.kind_of_seed(s) for s in seeds}
    assert kinds == {"pdf", "scatter", "plain_pdf", "plain_scatter"}


def test_every_listed_case_is_hit(oracle):
    """every carrier of every scene has >= 8 primary hits, and over the seeds every listed case is on such a carrier"""
    check_coverage(oracle, SEEDS)


def test_the_gpu_seeds_alone_meet_every_case(oracle):
    check_coverage(oracle, GPU_SEEDS)


def test_scatter_scenes_have_no_spec_diffuse():
    for seed in SEEDS:
        g, desc, cam, p = MG.scene(seed)
        has = any(desc.contents.materials[i].kind == MG.S for i in range(desc.contents.n_materials))
        assert has == (g.kind == "pdf")


def test_aov_and_guide_seeds_show_what_they_are_chosen_for():
    chains = {t for tags in tags_of(AOV_SEEDS) for t in tags if t[0] == "sd_chain"}
    assert {c[1] for c in chains} == {2, 3, MG.D_MAT} and {c[2] for c in chains} == {"spec", "diffuse", "mixed"}
    assert any(t[0] == "checker_depth" and t[1] >= 2 for tags in tags_of(AOV_SEEDS) for t in tags)
    inside = [tags for tags in tags_of(GUIDE_SEEDS) if any(t[0] == "pct" for t in tags)]          # carriers with a SpecDiffuse
    assert any(t[0] == "ref_idx" for tags in inside for t in tags), "a Dielectric inside a SpecDiffuse"
    assert any(t == ("fuzz", 0.0) for tags in inside for t in tags), "a Metal of fuzz 0 inside a SpecDiffuse"


@pytest.mark.parametrize("seed", AOV_SEEDS)
def test_first_hit_buffers_per_sample(seed, oracle, emu):
    g, desc, cam, p = MG.scene(seed)
    ref, _, features = aov_shared.run(oracle, emu, desc, cam, p, samples=(0, 1, 2, 3))
    aov_shared.assert_both_kinds_of_hit(ref)
    assert features & 0x40                        # the SpecDiffuse instance: aov_albedo's stack


@pytest.mark.parametrize("seed", GUIDE_SEEDS)
def test_guides_per_sample(seed, oracle, emu_guides):       # noqa: F811
    g, desc, cam, p = MG.scene(seed)
    guides_shared.run(oracle, emu_guides, desc, cam, p, fuzz_max=0.3)      # (Metals of fuzz 0 and 0.3 are followed)


@pytest.mark.parametrize("size", MG.IMAGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_image_edges_per_sample(size, oracle, emu):
    """u == 1 and v == 0 exactly, where u * width and (1 - v) * height are one past the last texel: on a rect on a coarse part of the
    f32 grid such hits are a few per cent of all (asserted from the oracle's first hits, not left to chance)"""
    d, desc, cam, p = MG.image_edge_scene(size)
    fh = oracle.first_hits(desc, cam, p, 0, p.samples_per_pixel)
    hit = fh["hit"] != 0
    for at_edge in (fh["u"][hit] == 1, fh["u"][hit] == 0, fh["v"][hit] == 1, fh["v"][hit] == 0):
        assert at_edge.sum() >= 8
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    img_e, ps_e, _, _ = emu.render_samples(desc, cam, p)
    compare(ps_o, ps_e, img_o, img_e)
