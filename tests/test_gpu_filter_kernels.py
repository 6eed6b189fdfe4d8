"""k_filter_prepare and k_filter_atrous<1..3> (both tap sources: LDS tile and L1 / L2) against the float64 restatement
(tests/filter_ref.py), through the unit entry lh2_core_filter_unit, on seeded synthetic buffers of 37 x 21 and 70 x 9:
partial tiles, step-4 taps (reaching 8 pixels) across both borders, rows where the v bound skips taps and the u clamp
duplicates them.  The buffers hold two material ids, a depth discontinuity, a normal edge, history counts 0 and 15, some
pixels with a negative moment variance (every tap weight NaN -> 0), a specular patch, and a previous frame with a
disoccluded strip (other normals).

Tolerance.  e32 is the float32 restatement's largest error against float64 on the same inputs, relative to the
buffer's largest value, taken before the 5:11 packing; the kernel gets 4 x e32 (__expf and the order of a few sums
differ from numpy's float32, not by an order of magnitude), plus, for packed outputs, one unit of the packing
(1 / 2048: a value next to a step lands on either side).
Measured (seed 1, 37 x 21 | 70 x 9):
  e32      prepare shading 1.1e-07 | 1.1e-07, moments 9.3e-08 | 1.8e-07, motion 1.3e-07 | 1.3e-07;
           pass 1 2.4e-06 | 2.6e-06, pass 2 1.6e-06 | 1.3e-06, pass 3 (after remodulation) 8.7e-07 | 1.5e-06
  kernel   prepare shading 0 | 5.3e-05 (one packing unit; bound 5.4e-05), moments 9.3e-08 | 1.8e-07, motion 1.3e-07 | 1.3e-07:
           the float32 restatement's own figures; pass 1 1.92e-04 | 1.87e-04 (bound 2.01e-04 | 1.98e-04) and pass 2
           1.88e-04 | 1.86e-04 (bound 1.94e-04 | 1.92e-04): one packing unit on a few values; pass 3 8.7e-07 | 1.5e-06
           (bound 3.5e-06 | 6.1e-06).  The LDS and the L1 / L2 variant give the same figures.  
Pixels with a tap whose weight is finite in one precision and not in the other may be left out, at most 0.5 %: the CPU
test below checks that the float32 restatement alone stays within that cap (it has none)."""
import numpy as np
import pytest

import filter_ref as R

SIZES = [(37, 21), (70, 9)]
SEED = 1


def make_buffers(w, h, seed=SEED):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    f = np.float32
    # a pinhole camera looking down +z; the previous one sits a little to the left
    aspect = w / h
    view = (np.array([0, 0, -4], f), np.array([-aspect, 1, 0], f), np.array([aspect, 1, 0], f), np.array([-aspect, -1, 0], f))
    prev = tuple(v + np.array([0.12, -0.05, 0.0], f) for v in view)
    # depth: a slanted plane with a step; normals: two halves
    depth = (5 + 0.05 * xs + 0.02 * ys + np.where(xs > 0.6 * w, 3.0, 0.0)).astype(f)
    n_a, n_b, n_c = np.array([0, 0, -1], f), np.array([0.6, 0, -0.8], f), np.array([1, 0, 0], f)
    normal = np.where((ys > h // 2)[..., None], n_b, n_a).astype(f)
    mat = np.where(xs < w // 3, 1, 2).astype(np.uint32)
    count = np.where(((xs // 5) + (ys // 4)) % 2 == 0, 15, 0).astype(np.uint32)
    spec = ((xs >= 15) & (xs < 18) & (ys >= 1) & (ys < 4)).astype(np.uint32)
    features = np.zeros((h, w, 4), np.uint32)
    features[..., 0] = R.pack_rgb(rng.uniform(0.2, 1.0, (h, w, 3)))
    features[..., 1] = R.pack_normal(normal) + spec
    features[..., 2] = depth.view(np.uint32)
    features[..., 3] = count + (spec << 4) + (mat << 6)
    D = view[1] + ((xs + 0.5) / w)[..., None] * (view[2] - view[1]) + ((ys + 0.5) / h)[..., None] * (view[3] - view[1]) - view[0]
    D = (D / np.linalg.norm(D, axis=-1, keepdims=True)).astype(f)
    worldPos = np.zeros((h, w, 4), f)
    worldPos[..., :3] = view[0] + depth[..., None] * D
    worldPos[..., 3] = features[..., 1].view(f)
    # the previous frame: the same surfaces seen from prev (nearest pixel), but a strip with another normal
    prevWorldPos = worldPos.copy()
    prevWorldPos[..., :3] += rng.normal(0, 0.01, (h, w, 3)).astype(f)
    strip = (xs >= 8) & (xs < 12)
    pn = (R.pack_normal(np.broadcast_to(n_c, (h, w, 3))) + spec).astype(np.uint32)
    prevWorldPos[..., 3] = np.where(strip, pn, features[..., 1]).astype(np.uint32).view(f)
    # ... and around the specular patch a specular surface that moved 3 pixels right and 1 down: its search has one clear minimum
    block = (xs >= 13) & (xs < 25) & (ys >= 1) & (ys < 7)
    moved = np.roll(worldPos, (1, 3), axis=(0, 1))
    prevWorldPos[block, :3] = moved[block, :3]
    moved_n = (np.roll(features[..., 1], (1, 3), axis=(0, 1)) & ~np.uint32(3)) | 1
    prevWorldPos[..., 3] = np.where(block, moved_n, prevWorldPos[..., 3].view(np.uint32)).astype(np.uint32).view(f)
    deltaDepth = np.zeros((h, w, 4), f)
    deltaDepth[..., 2], deltaDepth[..., 3] = 0.05, 0.02
    acc = np.zeros((2, h, w, 4), f)
    acc[0, ..., :3] = rng.uniform(0, 3.0, (h, w, 3))      # some above the direct clamp once demodulated
    acc[1, ..., :3] = rng.uniform(0, 2.0, (h, w, 3))
    m1, m3 = rng.uniform(0.1, 1.0, (h, w)), rng.uniform(0.1, 1.0, (h, w))
    var = np.where(rng.random((h, w)) < 0.03, -0.05, rng.uniform(0.01, 0.3, (h, w)))
    moments = np.stack([m1, m1 * m1 + var, m3, m3 * m3 + np.abs(var)], -1).astype(f)
    prevMoments = np.stack([m3, m3 * m3 + 0.1, m1, m1 * m1 + 0.2], -1).astype(f)
    A = R.combine(rng.uniform(0, 2.5, (h, w, 3)), rng.uniform(0, 3.0, (h, w, 3)), np.float64)
    B = R.combine(rng.uniform(0, 2.5, (h, w, 3)), rng.uniform(0, 3.0, (h, w, 3)), np.float64)
    # motion for the first pass: a smooth shift, off the frame at the right and bottom edges
    motion = np.stack([xs + 0.5 + 0.8, ys + 0.5 + 0.3], -1).astype(f)
    return dict(view=view, prev=prev, features=features, worldPos=worldPos, prevWorldPos=prevWorldPos, deltaDepth=deltaDepth, acc=acc,
                moments=moments, prevMoments=prevMoments, A=A, B=B, motion=motion)


def ref_prepare(b, dt, h):
    return R.prepare(b["acc"], b["features"], b["worldPos"], b["prevWorldPos"], b["deltaDepth"], b["prevMoments"], R.prev_view(b["prev"], h),
                     R.prev_view(b["view"], h), dt, cam_stationary=False)


def ref_atrous(b, phase, dt):
    return R.atrous(phase, b["features"], b["worldPos"], b["prevWorldPos"], b["deltaDepth"], b["motion"], b["moments"], b["A"], b["B"], dt)


def flipped(b, phase):
    """Pixels with a tap weight finite in one precision only."""
    f64, f32 = ref_atrous(b, phase, np.float64), ref_atrous(b, phase, np.float32)
    return (f64["finite"] != f32["finite"]).any(axis=(2, 3)), f64, f32


@pytest.mark.parametrize("w,h", SIZES)
def test_float32_restatement_error_and_exclusions(w, h):
    """CPU: the float32 restatement's own error (the tolerances' base) and the share of excluded pixels."""
    b = make_buffers(w, h)
    p64, p32 = ref_prepare(b, np.float64, h), ref_prepare(b, np.float32, h)
    assert np.array_equal(p64["found"], p32["found"]) and np.array_equal(p64["features"], p32["features"])
    assert 0.2 < p64["found"].mean() < 0.98                                 # some pixels have history, some are disoccluded
    e = {k: R.rel_max(p32[k], p64[k]) for k in ("direct", "indirect", "moments", "motion")}
    print(f"{w}x{h} prepare e32 {e}")
    assert max(e.values()) < 2e-6
    for phase in (1, 2, 3):
        ex, f64, f32 = flipped(b, phase)
        assert ex.mean() <= 0.005, (phase, ex.mean())
        assert not f64["finite"].all()                                      # the NaN weights are there
        keep = ~ex
        e32 = max(R.rel_max(f32["direct"][keep], f64["direct"][keep]), R.rel_max(f32["indirect"][keep], f64["indirect"][keep]))
        print(f"{w}x{h} pass {phase} e32 {e32:.2e} excluded {ex.mean():.4f}")
        assert e32 < 2e-5


def _view(v):
    from lighthouse2_amd import abi
    out = abi.ViewPyramid()
    out.pos, out.p1, out.p2, out.p3 = (abi.float3(*map(float, x)) for x in v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_prepare_matches_restatement(core, w, h):
    b = make_buffers(w, h)
    p64, p32 = ref_prepare(b, np.float64, h), ref_prepare(b, np.float32, h)
    g = core.filter_unit(0, features=b["features"], worldPos=b["worldPos"], prevWorldPos=b["prevWorldPos"], deltaDepth=b["deltaDepth"],
                         acc=b["acc"], prevMoments=b["prevMoments"], prev_view=_view(b["prev"]), view=_view(b["view"]), cam_stationary=False)
    assert np.array_equal(g["features"], p64["features"])                 # the history counts
    peak = float(np.max(R.unpacked(p64["shading"])))
    e32 = max(R.rel_max(p32["direct"], p64["direct"]), R.rel_max(p32["indirect"], p64["indirect"]))
    err = R.rel_max(R.unpacked(g["shading"]), R.unpacked(p64["shading"]))
    print(f"{w}x{h} prepare shading: kernel {err:.2e}, e32 {e32:.2e}, bound {4 * e32 + R.STEP / peak:.2e}")
    assert err <= 4 * e32 + R.STEP / peak
    for k in ("moments", "motion"):
        e32, err = R.rel_max(p32[k], p64[k]), R.rel_max(g[k], p64[k])
        print(f"{w}x{h} prepare {k}: kernel {err:.2e}, e32 {e32:.2e}")
        assert err <= 4 * e32, k


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("phase", [1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_atrous_matches_restatement(core, w, h, phase, lds):
    b = make_buffers(w, h)
    ex, f64, f32 = flipped(b, phase)
    assert ex.mean() <= 0.005
    keep = ~ex
    g = core.filter_unit(phase, features=b["features"], worldPos=b["worldPos"], prevWorldPos=b["prevWorldPos"], deltaDepth=b["deltaDepth"],
                         motion=b["motion"], moments=b["moments"], in_=b["A"], prev=b["B"], lds=bool(lds))["out"]
    if phase == 3:
        e32 = R.rel_max(f32["out"][keep][:, :3], f64["out"][keep][:, :3])
        err = R.rel_max(g[keep][:, :3], f64["out"][keep][:, :3])
        bound = 4 * e32
        assert np.array_equal(g[..., 3], np.ones((h, w), np.float32))
    else:
        e32 = max(R.rel_max(f32["direct"][keep], f64["direct"][keep]), R.rel_max(f32["indirect"][keep], f64["indirect"][keep]))
        ref = R.unpacked(f64["out"])[keep]
        err = R.rel_max(R.unpacked(g)[keep], ref)
        bound = 4 * e32 + R.STEP / float(np.max(ref))
    print(f"{w}x{h} pass {phase} lds {lds}: kernel {err:.2e}, e32 {e32:.2e}, bound {bound:.2e}, excluded {int(ex.sum())}")
    assert err <= bound
