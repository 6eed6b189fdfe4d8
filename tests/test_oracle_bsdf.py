"""The CPU oracle's Disney BSDF (orc_evaluate_bsdf / orc_sample_bsdf: its material packing, its ShadingData and its
EvaluateBSDF / SampleBSDF) against the float64 restatement written from the reference's text (tests/bsdf_ref.py), and the
sensitivity of scene.disney_scene to each of its materials' parameters.

Inputs (bsdf_ref.make_inputs, seed 7): 20000 random samples over the materials of disney_scene plus the edge materials,
about 12 % of the directions grazing, 10 % of the wow below N; then the edge list: every material x {plain, wo.z == 0
exactly, wi.z == 0 exactly, wow below N, from inside past TIR, iN != N, wow below iN but above N, wo.z == 1} x r0 in {0,
just under TRANSMISSION, just under 1, nine values between} x two r1, and r3 on each cdf boundary and one step to each side
of it.  The edge
materials add eta 1, roughness byte 0, anisotropic 1, clearcoatGloss 0 and 1, metallic 1, subsurface exactly 1 and a
glass with absorption; the scene brings the all-parameters, the half-transmission and the all-zero-weight material.

Bound.  The error of an output is taken per sample and component, relative to max(|reference|, the batch median of
|reference|).  e32 is the float32 restatement's worst such error over the kept samples of a class; the oracle gets 4 x e32,
as the filter tests give their kernels: lh2_logf / lh2_powf / lh2_sincosf / lh2_expf differ from numpy's float32 functions,
not by an order of magnitude (measured: the oracle's figures equal e32 to the printed digits, so no larger factor is
needed).  The same rule is asserted on the 99th percentile, which one ill-conditioned sample cannot widen.  The classes
(groups()): the scene's materials on the random samples, the scene's materials on the edge list, and the edge materials,
which sit where float32 itself is far from float64 (see groups()).  Samples whose branch decisions differ between the
float32 and the float64 restatement ("flipped") are left out, at most 0.5 % of the batch for EvaluateBSDF and 2 % for
SampleBSDF; a sample whose wiw is left unset compares value, pdf and the flag only.
Measured (seed 7, 20000 + 4392 samples; worst e32 = oracle, bound 4 x; [99th percentile]):
  EvaluateBSDF, flipped 0
    scene materials, random      value 1.73e-04 [1.1e-06]   pdf 1.96e-04 [8.9e-07]
    scene materials, edge list   value 1.03e-06 [6.6e-07]   pdf 1.32e-06 [1.3e-06]
    edge materials               value 1.06e-04 [3.0e-06]   pdf 1.59e-04 [3.0e-06]
  SampleBSDF, flipped 0.0128 (312 samples, all on the edge list: r0 on a cdf boundary or one step under TRANSMISSION)
    scene materials, random      value 1.88e-04 [8.9e-06]   pdf 8.08e-04 [1.0e-05]   wiw 4.88e-04 [2.6e-06]
    scene materials, edge list   value 2.41e-01 [2.0e-03]   pdf 1.23e-01 [1.8e-03]   wiw 6.70e-02 [1.1e-03]
    edge materials               value 5.74e-01 [9.6e-02]   pdf 5.74e-01 [9.6e-02]   wiw 8.99e-02 [1.4e-05]
  the specular flag is equal everywhere.  DESIGN.md section 3 has the same figures.

Sensitivity.  disney_scene at 160 x 96, 2 spp, on the oracle: unsetting (1e-32) any parameter a material is about moves
the accumulator over that material's primary-hit pixels (501 - 548 of them) by rel-L2 >= 1e-2, 100 x the frame parity
bar, so frame parity on this scene tests the parameter.  Measured: 3.4e-02 (subsurface on the all-parameters material),
5.2e-02 (specularTint there), 5.9e-02 (specular on the metal), every other one >= 1.7e-01.  The parameters a material is
not about hold filler bytes 0 .. 9, there only to make its eleven bytes pairwise distinct; they are not unset here."""
import functools

import numpy as np
import pytest

import bsdf_ref as R
from lighthouse2_amd import abi, scene
from oracle.oracle import Oracle

CAP = {"evaluate": 0.005, "sample": 0.02}
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def unit_materials():
    return tuple(scene.disney_materials()[0] + R.edge_materials())


@functools.lru_cache(maxsize=None)
def inputs():
    return R.make_inputs(list(unit_materials()))


@functools.lru_cache(maxsize=None)
def restatement(mode: str, dtname: str):
    """bsdf_ref on the shared inputs, computed once per (mode, float type) and left unchanged."""
    dt = np.float64 if dtname == "f64" else np.float32
    x = inputs()
    M = R.convert_materials(list(unit_materials()))
    sd = R.shading_data(M, x["material"], x["wow"], x["N"], dt)
    if mode == "evaluate":
        out = R.evaluate_bsdf(sd, x["iN"], x["iT"], x["wow"], x["wiw"], dt)
    else:
        out = R.sample_bsdf(sd, x["iN"], x["N"], x["iT"], x["wow"], x["distance"], x["r0"], x["r1"], dt)
    for v in out.values():
        v.setflags(write=False)
    return out


def records(mode: str):
    x = inputs()
    return abi.bsdf_records(x["material"], x["iN"], x["N"], x["iT"], x["wow"], wiw=x["wiw"], r0=x["r0"], r1=x["r1"], distance=x["distance"])


def groups():
    """The three classes of samples an error bound is taken over.  The edge materials sit where the model is ill-conditioned
    on purpose: roughness byte 0 and clearcoatGloss 1 put a microfacet alpha at its 0.001 clamp, where the lobe amplifies a
    rounding of the half vector by 1 / alpha^2 = 1e6, and eta 1 refracts grazing rays through 1 - sin^2 = 1e-6.  Their
    float32 error would set a bound of order 1 for everything, so the scene's materials get bounds of their own, the
    random samples and the edge list (exact zeros, cdf boundaries) apart."""
    x = inputs()
    extra = x["material"] >= len(scene.disney_materials()[0])
    rnd = np.arange(len(extra)) < x["n_random"]
    return {"scene materials, random": rnd & ~extra, "scene materials, edge list": ~rnd & ~extra, "edge materials": extra}


def check_against_restatement(mode: str, got: np.ndarray, who: str):
    """`got`: (n, 8) unit-entry output.  Asserts the exclusion cap, then got against float64 within FACTOR x e32 per output
    and group; returns the figures."""
    f64, f32 = restatement(mode, "f64"), restatement(mode, "f32")
    ex = R.flipped(f32["dec"], f64["dec"])
    share = float(ex.mean())
    assert share <= CAP[mode], (mode, share)
    keep = ~ex
    outs = {"value": (got[:, 0:3], keep), "pdf": (got[:, 3], keep)}
    if mode == "sample":
        outs["wiw"] = (got[:, 4:7], keep & f64["wiw_set"] & f32["wiw_set"])
        flag = got[:, 7].view(np.uint32)
        assert np.array_equal(flag[keep] != 0, f64["specular"][keep]), "specular flag"
        assert set(np.unique(flag)) <= {0, 1}
    print(f"{mode}: excluded {share:.4f} ({int(ex.sum())} of {len(ex)})")
    fig = {}
    for name, (g, k) in outs.items():
        a32, a = R.rel_err(f32[name], f64[name], k), R.rel_err(g, f64[name], k)
        for gname, gm in groups().items():
            sel = k & gm
            e32, err = float(a32[sel].max()), float(a[sel].max())
            p32, perr = float(np.percentile(a32[sel], 99)), float(np.percentile(a[sel], 99))
            fig[name, gname] = (e32, err, p32, perr)
            print(f"{mode} {name}, {gname} ({int(sel.sum())}): worst e32 {e32:.2e}, {who} {err:.2e}, bound {FACTOR * e32:.2e}; "
                  f"99th percentile e32 {p32:.2e}, {who} {perr:.2e}")
    for key, (e32, err, p32, perr) in fig.items():
        assert np.isfinite(e32) and err <= FACTOR * e32, (mode, key, err, e32)
        assert perr <= FACTOR * p32, (mode, key, perr, p32)          # the same rule on the 99th percentile: the bulk, not one sample
    return fig


@pytest.fixture(scope="module")
def orc():
    o = Oracle()
    o.set_materials(list(unit_materials()))
    yield o
    o.close()


def test_material_bytes_are_distinct():
    """Every Disney material of the scene (the black one apart) has eleven pairwise distinct parameter bytes, and every
    parameter is featured by some material."""
    mats, featured = scene.disney_materials()
    M = R.convert_materials(mats)
    seen = set()
    for mi, par in featured.items():
        seen |= set(par)
        if par:
            assert len(set(M["byte"][mi].tolist())) == 11, (mi, M["byte"][mi])
        else:
            assert not M["byte"][mi].any() and not M["color"][mi].any()
    assert seen == set(R.PARAMS)
    assert any(len(par) == 11 for par in featured.values())


@pytest.mark.parametrize("mode", ["evaluate", "sample"])
def test_float32_restatement_flips_and_branches(mode):
    """The float32 restatement alone stays within the exclusion caps, and the inputs reach every branch."""
    f64, f32 = restatement(mode, "f64"), restatement(mode, "f32")
    ex = R.flipped(f32["dec"], f64["dec"])
    print(f"{mode}: flipped {ex.mean():.4f} ({int(ex.sum())} of {len(ex)})")
    assert ex.mean() <= CAP[mode]
    names = R.DECISIONS_EVAL if mode == "evaluate" else R.DECISIONS_SAMPLE
    d = f64["dec"]
    for k, name in enumerate(names):
        vals = set(np.unique(d[:, k]).tolist()) - {-1}
        want = {0, 1, 2, 3} if name == "lobe" else {0, 1}
        if name in ("coat_zero_exit", "spec_zero_exit", "mf_wi_zero", "refract_tir"):
            want = {0}     # the early exits need wi.z == 0 from the sampler, or the two TIR tests to disagree: not required
        assert want <= vals, (mode, name, vals)
    if mode == "sample":
        assert (~f64["wiw_set"]).sum() > 0
        x = inputs()
        black = [i for i, p in scene.disney_materials()[1].items() if not p][0]
        b = x["material"] == black
        assert np.all(f64["pdf"][b] == 0) and np.all(restatement("evaluate", "f64")["pdf"][b] == 0)


def test_oracle_evaluate_matches_float64(orc):
    check_against_restatement("evaluate", orc.bsdf_unit(False, records("evaluate")), "oracle")


def test_oracle_sample_matches_float64(orc):
    check_against_restatement("sample", orc.bsdf_unit(True, records("sample")), "oracle")


def test_evaluate_sheen_overwrites_diffuse(orc):
    """disney.h:315-316: with a sheen weight, the value EvaluateBSDF returns holds no diffuse term.  The oracle follows the
    text, not the sum with the diffuse term a reader would expect."""
    mats, featured = scene.disney_materials()
    mi = [i for i, p in featured.items() if "sheen" in p and len(p) < 11][0]
    x = inputs()
    sel = np.flatnonzero((x["material"] == mi) & (np.arange(len(x["material"])) < x["n_random"]))
    as_text = restatement("evaluate", "f64")["value"][sel]
    M = R.convert_materials(list(unit_materials()))
    sd = R.shading_data(M, x["material"][sel], x["wow"][sel], x["N"][sel], np.float64)
    d = lambda k: x[k][sel].astype(np.float64)
    _, diffuse = R._Ops(np.float64).evaluate_diffuse(sd, d("iN"), d("wow"), d("wiw"))
    got = orc.bsdf_unit(False, records("evaluate")[sel])[:, :3]
    near = np.linalg.norm(got - as_text) / np.linalg.norm(as_text)
    far = np.linalg.norm(got - (as_text + diffuse)) / np.linalg.norm(as_text)
    print(f"sheen material: oracle to the text's value {near:.1e}, to the value with the diffuse term {far:.1e}")
    assert near < 1e-5 and far > 1e-2


# ---- sensitivity of disney_scene ----------------------------------------------------------------
W, H, SPP = 160, 96, 2


def primary_materials(orc, sc):
    """Material index of each pixel's primary hit (-1: miss), from trace_closest on the frame's eye rays."""
    o, d, _ = orc.generate_eye_rays(sc.view, 0, 0)
    hits = orc.trace_closest(o, d)
    tri = hits[:, 1].view(np.int32)
    mat = np.where(tri >= 0, sc.meshes[0].view(np.uint32)[np.maximum(tri, 0), abi.TRI["material"]].astype(np.int64), -1)
    return mat.reshape(H, W)


def render(orc, sc):
    orc.set_materials(sc.materials)
    orc.set_target(W, H, SPP)
    sc.render_frame(orc)
    return orc.accumulator().astype(np.float64)


def test_disney_scene_is_sensitive_to_every_parameter():
    """Measured rel-L2 over the material's own pixels when the parameter is unset (region sizes 500 - 800 pixels): the
    figures are printed; the smallest are listed in DESIGN.md section 3."""
    sc = scene.disney_scene(W, H)
    orc = Oracle()
    try:
        sc.load_into(orc)
        orc.set_target(W, H, 1)
        region = primary_materials(orc, sc)
        base = render(orc, sc)
        assert np.isfinite(base).all()
        worst = []
        for mi, par in sc.featured.items():
            px = region == mi
            assert px.sum() >= 200, (mi, int(px.sum()))
            for name in par:
                mats = list(sc.materials)
                m = abi.CoreMaterial.from_buffer_copy(bytes(mats[mi]))
                getattr(m, name).value = 1e-32
                mats[mi] = m
                alt = scene.Scene(**{**sc.__dict__, "materials": mats})
                a = render(orc, alt)
                rel = float(np.linalg.norm((a - base)[px][:, :3]) / np.linalg.norm(base[px][:, :3]))
                print(f"material {mi} ({int(px.sum())} px) without {name}: rel-L2 {rel:.2e}")
                worst.append((rel, mi, name))
        bad = [w for w in worst if not w[0] >= 1e-2]
        assert not bad, bad
    finally:
        orc.close()
