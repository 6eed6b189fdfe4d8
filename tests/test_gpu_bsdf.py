"""The Disney BSDF of the shade kernels on the GPU: the unit entry lh2_core_bsdf_unit (k_bsdf_unit calls the SampleBSDF /
EvaluateBSDF device functions the shade kernels call, on ShadingData unpacked from the core's own uploaded material
records) and frames of scene.disney_scene, whose materials reach every lobe and every parameter byte.

Unit, against the CPU oracle (orc_evaluate_bsdf / orc_sample_bsdf), on the inputs of tests/test_oracle_bsdf.py (20000 random
samples and the edge list over the scene's and the edge materials): value, pdf and the specular flag equal bit for bit, wiw
where pdf > 0, NaN matching NaN: what include/lh2_detmath.h promises.  Against the float64 restatement (tests/bsdf_ref.py):
the bound and the exclusions of test_oracle_bsdf.py, where the figures are listed (the kernel's are the oracle's, bit for bit).

Frames, against the oracle at 160 x 96, two frames at 2 spp: identical ray counts, rel-L2 <= 1e-4 on rgb and <= 1e-6 on w over
the frame, and rel-L2 <= 1e-4 over each material's primary-hit pixels apart; with maxPathLength 2 (k_shade_last) and 5, a
launch pair per bounce and the path tail from bounce 2 (both kernel variants); with the denoise mode's capture the two planes
sum to the filter-off accumulator; the frame is finite everywhere, the black material's pixels included.
Measured (MI355X): unit bit for bit on all 24392 samples of both modes; against float64 the kernel's figures are the oracle's
(test_oracle_bsdf.py).  Frames: rel-L2 rgb 3.8e-08 .. 4.1e-08, w 0; per material region (maxPathLength 5, no tail) floor
3.6e-08, wall 4.0e-08, sheen 3.9e-08, clearcoat 3.7e-08, anisotropic metal 4.7e-08, subsurface 3.5e-08, specularTint 4.0e-08,
all parameters 4.1e-08, half glass 4.0e-08, black 0 (its pixels are exactly 0 on both sides); the other five cases lie
between 2.6e-08 and 4.4e-08; planes against the accumulator 3.9e-08, w 0.  """
import functools

import numpy as np
import pytest

import test_oracle_bsdf as T
from lighthouse2_amd import scene
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

W, H, SPP = T.W, T.H, T.SPP


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def unit_core(core):
    core.set_materials(list(T.unit_materials()))
    return core


@pytest.mark.parametrize("mode", ["evaluate", "sample"])
def test_unit_matches_oracle_bit_for_bit(unit_core, mode):
    rec = T.records(mode)
    o = Oracle()
    try:
        o.set_materials(list(T.unit_materials()))
        want = o.bsdf_unit(mode == "sample", rec)
    finally:
        o.close()
    got = unit_core.bsdf_unit(mode == "sample", rec)
    gu, wu = got.view(np.uint32), want.view(np.uint32)
    same = (gu == wu) | (np.isnan(got) & np.isnan(want))
    cols = [0, 1, 2, 3, 7] if mode == "sample" else [0, 1, 2, 3]
    bad = np.flatnonzero(~same[:, cols].all(axis=1))
    assert bad.size == 0, (mode, bad[:10], got[bad[:3]], want[bad[:3]], T.inputs()["material"][bad[:10]])
    if mode == "sample":
        live = want[:, 3] > 0
        bad = np.flatnonzero(live & ~same[:, 4:7].all(axis=1))
        assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
        assert live.sum() > 0.5 * len(live)


@pytest.mark.parametrize("mode", ["evaluate", "sample"])
def test_unit_matches_float64(unit_core, mode):
    T.check_against_restatement(mode, unit_core.bsdf_unit(mode == "sample", T.records(mode)), "kernel")


def test_unit_rejects_a_material_out_of_range(unit_core):
    rec = T.records("evaluate")[:4].copy()
    rec.view(np.int32)[2, 3] = len(T.unit_materials())
    with pytest.raises(Exception, match="material"):
        unit_core.bsdf_unit(False, rec)


# ---- frames ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_frames(depth: int):
    """Two frames of disney_scene at 2 spp on the oracle (computed once per depth, left unchanged), and the material of each
    pixel's primary hit."""
    sc = scene.disney_scene(W, H)
    o = Oracle()
    try:
        sc.load_into(o)
        o.set_target(W, H, 1)
        region = T.primary_materials(o, sc)
        o.set_target(W, H, SPP)
        o.setting("maxPathLength", depth)
        counts = []
        for f in range(2):
            sc.render_frame(o, converge=1 if f == 0 else 0)
            counts.append(o.ray_counts())
        acc = o.accumulator()
    finally:
        o.close()
    acc.setflags(write=False)
    return sc, region, counts, acc


def check_frame(acc, depth, what):
    sc, region, _, ref = oracle_frames(depth)
    assert np.isfinite(acc).all()
    whole, whole_w = rel_l2(acc[..., :3], ref[..., :3]), rel_l2(acc[..., 3], ref[..., 3])
    per = {}
    for mi in sorted(set(sc.featured) | {0, 1}):
        px = region == mi
        assert px.sum() >= 200, (mi, int(px.sum()))
        n = np.linalg.norm(ref[px][:, :3])
        # the black material's region holds what passes through it alone; a region of zeros compares equal or not at all
        per[mi] = rel_l2(acc[px][:, :3], ref[px][:, :3]) if n > 0 else float(np.abs(acc[px][:, :3]).max())
    print(f"{what}: frame rel-L2 rgb {whole:.2e} w {whole_w:.2e}; per material " + ", ".join(f"{k}: {v:.1e}" for k, v in per.items()))
    assert whole <= 1e-4 and whole_w <= 1e-6, (whole, whole_w)
    assert max(per.values()) <= 1e-4, per


@pytest.mark.parametrize("tail,waves", [(0, 0), (2, 0), (2, 4)])
@pytest.mark.parametrize("depth", [2, 5])
def test_disney_scene_frame_parity(fresh_core, depth, tail, waves):
    sc, _, counts, _ = oracle_frames(depth)
    sc.load_into(fresh_core)
    fresh_core.set_target(W, H, SPP)
    fresh_core.setting("maxPathLength", depth)
    fresh_core.setting("pathTail", tail)
    fresh_core.setting("pathTailWaves", waves)
    for f in range(2):
        sc.render_frame(fresh_core, converge=1 if f == 0 else 0)
        cg = fresh_core.ray_counts()
        assert np.array_equal(cg, counts[f]), (f, cg[:8], counts[f][:8])
    assert counts[1][1] > 0 and counts[1][16] > 0
    check_frame(fresh_core.accumulator(), depth, f"maxPathLength {depth}, pathTail {tail}, waves {waves}")


def test_disney_scene_filter_planes(fresh_core):
    """The denoise mode's capture on this scene: plane 0 + plane 1 is the filter-off accumulator, and that is the oracle's."""
    depth = 5
    sc, _, counts, _ = oracle_frames(depth)
    sc.load_into(fresh_core)
    fresh_core.set_target(W, H, SPP)
    fresh_core.setting("maxPathLength", depth)
    fresh_core.setting("filter", 0)
    sc.render_frame(fresh_core)
    off, c_off = fresh_core.accumulator(), fresh_core.ray_counts()
    fresh_core.setting("filter", 1)
    sc.render_frame(fresh_core)
    planes, c_on = fresh_core.filter_buffer("acc"), fresh_core.ray_counts()
    fresh_core.setting("filter", 0)
    total = planes[0] + planes[1]
    assert np.isfinite(total).all()
    rel, rel_w = rel_l2(total[..., :3], off[..., :3]), rel_l2(total[..., 3], off[..., 3])
    print(f"planes vs accumulator rel-L2 rgb {rel:.2e} w {rel_w:.2e}")
    assert rel <= 1e-4 and rel_w <= 1e-4
    assert np.array_equal(c_off, c_on) and np.array_equal(c_off, counts[0])
