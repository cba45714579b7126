"""-m gpu: the randomised material and texture graphs of tests/material_graphs.py on the MI355X, through the C ABI, against the
oracle: radiance and draw counts per sample (test_gpu_parity.compare_samples), the first-hit buffers (test_gpu_aov's comparison) and
the guides (test_guides_gpu's), on the seeds tests/test_material_graphs.py runs on the CPU; the chains at the nesting limits; and the
launch log, which must show the Cornell-type instances for the plain scenes and the everything-instances for the others.  Every
description here is one the lineariser accepts: what it must refuse is tested on the CPU alone (tests/test_validation.py)."""
import pytest

import material_graphs as MG
import test_material_graphs as cpu
from test_gpu_aov import _check_against_a
from test_gpu_parity import compare_samples, device_samples
from test_guides_gpu import check as check_guides
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu

F_CORNELL, F_ALL, F_PDF = 0x116, 0x17F, 0x80


def per_sample(desc, cam, p, oracle):
    ds = DeviceScene(desc)
    try:
        img_d, ps_d = device_samples(ds, cam, p)
        log = ffi.last_launches(ds._lib, ds._h)
    finally:
        ds.close()
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    compare_samples(ps_o, ps_d, img_o, img_d)
    return {r.features for r in log}


@pytest.mark.parametrize("seed", cpu.GPU_SEEDS)
def test_material_graph_per_sample(seed, device, oracle):
    g, desc, cam, p = MG.scene(seed)
    launched = per_sample(desc, cam, p, oracle)
    assert launched == {(F_CORNELL if g.plain else F_ALL) | (F_PDF if g.use_pdf else 0)}, [hex(f) for f in launched]


def test_the_seeds_meet_every_case_and_every_instance(oracle):
    cpu.check_coverage(oracle, cpu.GPU_SEEDS)
    kinds = [MG.kind_of_seed(s) for s in cpu.GPU_SEEDS]
    assert kinds.count("plain_pdf") >= 1 and kinds.count("plain_scatter") >= 1 and kinds.count("scatter") >= 1


@pytest.mark.parametrize("seed", cpu.AOV_SEEDS)
def test_first_hit_buffers_per_sample(seed, device, oracle):
    g, desc, cam, p = MG.scene(seed)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle, samples=(0, 1, 2, 3))
    finally:
        ds.close()


@pytest.mark.parametrize("seed", cpu.GUIDE_SEEDS)
def test_guides_per_sample(seed, device, oracle):
    g, desc, cam, p = MG.scene(seed)
    check_guides(desc, cam, p, oracle, fuzz_max=0.3)


def test_checker_chain_at_the_limit(device, oracle):
    d, desc, cam, p = MG.checker_chain_scene(MG.D_TEX)
    assert per_sample(desc, cam, p, oracle) == {F_ALL | F_PDF}


@pytest.mark.parametrize("side", ["spec", "diffuse", "mixed"])
def test_spec_diffuse_chain_at_the_limit(side, device, oracle):
    d, desc, cam, p = MG.spec_diffuse_chain_scene(MG.D_MAT, side)
    assert per_sample(desc, cam, p, oracle) == {F_ALL | F_PDF}
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
    finally:
        ds.close()
