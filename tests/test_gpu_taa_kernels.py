"""k_filter_taa (both tap sources: LDS tile and L1 / L2) and k_filter_unsharpen (one variant: its LDS tile never won on
the GPU, profiles/r08_ab_taa_lds.txt, and was removed; it passed this test as the other does) against the float64 restatement
(tests/taa_ref.py), through the unit entry lh2_core_taa_unit, on seeded synthetic buffers of 37 x 21 and 70 x 9 (the
chain's sizes: partial tiles on both axes, two block rows) and 5 x 3 (almost everything is border).

Inputs.  A linear image of smooth gradients times uniform noise of +- 20 %, with a patch above 100 (the clamp at 10) and
one between 16 and 100 (the YCoCg clamp at 4); every 3 x 3 neighbourhood's variance in gamma space is at least 1e-3 of its
squared mean (asserted: below that var - avg^2 cancels in float32 and the comparison would measure the cancellation).  A
history image of the same kind, in gamma space, with one NaN pixel: every pixel whose 4 x 4 footprint holds it takes the
fallback, also where the tap's weight is zero.  Motion: a still region (pixel + 0.5 exactly: u is an integer), a smooth
shift of (0.8, 0.3), and two rows shifted by (-3.6, 2.7); footprints cross the left and the top edge and reach beyond the
right and the bottom one, and no u lies within 1e-3 of a frame bound (so the still region leaves out column 0 and row 0).
u is exact in float32, so no decision differs between the precisions: no pixel is excluded.

Tolerance, by the rule of tests/test_gpu_filter_kernels.py: e32 is the float32 restatement's largest error against
float64 on the same inputs, relative to the buffer's largest value; the kernel gets 4 x e32.  w is exact: 0 after the
pass, 1 after the unsharpen.  The pass's two tap sources must agree with each other to the same bound.
Measured on the CPU (seed 1; 37 x 21 | 70 x 9 | 5 x 3):
  e32      taa pass 2.8e-06 | 1.3e-06 | 6.7e-08; without history 2.4e-08 | 2.4e-08 | 2.3e-08; unsharpen 2.0e-07 | 1.4e-07 | 9.4e-08
The CPU test caps e32 at ten times these: it only catches a restatement that is not the same program in both precisions.
Measured on the GPU: every kernel error equals the float32 restatement's e32 to the printed digits, for both tap sources
(the kernels and numpy's float32 run the same operations in the same order).  """
import numpy as np
import pytest

import filter_ref as R
import taa_ref as T

SIZES = [(37, 21), (70, 9), (5, 3)]
SEED = 1
# the e32 measured on the CPU (the docstring's figures); the CPU test allows ten times as much
E32_MEASURED = {(37, 21): {"taa": 2.76e-06, "pass": 2.36e-08, "unsharpen": 2.01e-07},
                (70, 9): {"taa": 1.28e-06, "pass": 2.36e-08, "unsharpen": 1.39e-07},
                (5, 3): {"taa": 6.70e-08, "pass": 2.29e-08, "unsharpen": 9.43e-08}}


def _image(rng, w, h):
    """Linear radiance: smooth gradients x uniform noise of +- 20 %, a patch above 100 and one between 16 and 100."""
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs / max(w - 1, 1), ys / max(h - 1, 1)
    base = np.stack([0.25 + 0.5 * fx, 0.7 - 0.3 * fy, 0.3 + 0.25 * (fx + fy)], -1)
    px, py, pw, ph = w // 2, h // 3, max(1, w // 8), max(1, h // 4)
    hot = (xs >= px) & (xs < px + pw) & (ys >= py) & (ys < py + ph)                        # above 100: the clamp at 10
    warm = (xs >= px - 2 * pw) & (xs < px - pw) & (ys >= py) & (ys < py + ph)              # 16 .. 100: the YCoCg clamp at 4
    base = np.where(hot[..., None], np.array([200.0, 150.0, 300.0]), base)
    base = np.where(warm[..., None], np.array([40.0, 30.0, 50.0]), base)
    # the noise is uniform in +- 20 %, but stratified: nine strata laid out with period 3, so every 3 x 3 neighbourhood holds each
    # of them once and its variance is never small by chance (independent samples reach 2e-4 of the squared mean)
    tile = np.array([[0, 3, 7], [4, 6, 2], [8, 1, 5]])      # of all layouts the one whose 2 x 2 blocks (the frame's corners) spread most
    strata = np.stack([tile[(ys + c) % 3, (xs + 2 * c) % 3] for c in range(3)], -1)
    img = base * (0.8 + 0.4 * (strata + rng.uniform(0.0, 1.0, (h, w, 3))) / 9.0)
    return img, hot, warm


def make_buffers(w, h, seed=SEED):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    f = np.float32
    img, hot, warm = _image(rng, w, h)
    linear = np.concatenate([img, np.ones((h, w, 1))], -1).astype(f)
    assert (linear[hot][:, :3] > 100).all() and hot.any()
    assert ((linear[warm][:, :3] > 16) & (linear[warm][:, :3] < 100)).all() and warm.any()
    # the history: what a previous TAA pass could have written (gamma, at most 10, w = 0), and one NaN pixel
    pimg, _, _ = _image(rng, w, h)
    prev = np.concatenate([np.fmin(10.0, np.sqrt(pimg)), np.zeros((h, w, 1))], -1).astype(f)
    nan_at = (min(w - 1, w // 2 + 1), h // 2)                     # two to the right of the still region's last column
    prev[nan_at[1], nan_at[0], :3] = np.nan
    # motion: still (not in column 0 or row 0, where u would be a frame bound), a smooth shift elsewhere, two shifted rows
    still = (xs >= 1) & (xs < w // 2) & (ys >= 1)
    strip = (ys >= max(1, h - 4)) & (ys < max(2, h - 2))
    mx = np.where(still, xs + 0.5, xs + 0.5 + 0.8)
    my = np.where(still, ys + 0.5, ys + 0.5 + 0.3)
    mx, my = np.where(strip, xs + 0.5 - 3.6, mx), np.where(strip, ys + 0.5 + 2.7, my)
    motion = np.stack([mx, my], -1).astype(f)
    return dict(linear=linear, prev=prev, motion=motion, nan_at=nan_at, still=still & ~strip, strip=strip)


def _neighbourhood_variance_ok(linear):
    """Every 3 x 3 neighbourhood (its part inside the frame): variance in gamma space >= 1e-3 of its squared mean."""
    g = np.sqrt(linear[..., :3].astype(np.float64))
    h, w = g.shape[:2]
    worst = np.inf
    for y in range(h):
        for x in range(w):
            n = g[max(0, y - 1):y + 2, max(0, x - 1):x + 2].reshape(-1, 3)
            worst = min(worst, float(np.min(n.var(0) / n.mean(0) ** 2)))
    return worst


def _footprint_holds(b, w, h):
    """Pixels that blend with their history and whose 4 x 4 footprint holds the NaN pixel (weights not looked at)."""
    u = b["motion"][..., 0].astype(np.float64) - 0.5
    v = b["motion"][..., 1].astype(np.float64) - 0.5
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    x1, y1 = np.floor(u) - 1, np.floor(v) - 1
    nx, ny = b["nan_at"]
    return inside & (x1 <= nx) & (nx <= x1 + 3) & (y1 <= ny) & (ny <= y1 + 3), inside, u, v


@pytest.mark.parametrize("w,h", SIZES)
def test_inputs_and_float32_restatement(w, h):
    """CPU: the inputs have what the docstring says, both precisions take the same decisions, and e32 (the tolerances' base)."""
    b = make_buffers(w, h)
    worst = _neighbourhood_variance_ok(b["linear"])
    print(f"{w}x{h} smallest neighbourhood variance / mean^2 in gamma space: {worst:.2e}")
    assert worst >= 1e-3
    holds, inside, u, v = _footprint_holds(b, w, h)
    assert min(np.abs(u).min(), np.abs(u - w).min(), np.abs(v).min(), np.abs(v - h).min()) > 1e-3      # no u at a frame bound
    assert np.array_equal(u[b["still"]], np.mgrid[0:h, 0:w][1][b["still"]])                             # the still region: integers
    assert inside.any() and (~inside).any()
    x1, y1 = np.floor(u) - 1, np.floor(v) - 1
    assert (inside & (x1 < 0)).any() and (inside & (y1 < 0)).any()                                      # across the left and top edges
    assert (inside & (x1 + 3 >= w)).any() and (inside & (y1 + 3 >= h)).any()                            # beyond the right and bottom ones
    p64, p32 = T.taa_pass(b["linear"], b["prev"], b["motion"], True, np.float64), T.taa_pass(b["linear"], b["prev"], b["motion"], True, np.float32)
    for k in ("inside", "fallback"):
        assert np.array_equal(p64[k], p32[k]), k
    assert np.array_equal(p64["inside"], inside)
    assert np.array_equal(p64["fallback"], holds) and holds.any()
    # ... among them a still pixel two columns left of the NaN: its tap there has weight 0
    nx, ny = b["nan_at"]
    assert (holds & b["still"] & (np.floor(u) + 2 == nx)).any()
    assert not np.isnan(p64["out"]).any()
    n64, n32 = T.taa_pass(b["linear"], b["prev"], b["motion"], False, np.float64), T.taa_pass(b["linear"], b["prev"], b["motion"], False, np.float32)
    assert not n64["inside"].any() and not n32["inside"].any()
    assert np.array_equal(n64["out"][..., :3], np.fmin(10.0, np.sqrt(b["linear"][..., :3].astype(np.float64))))
    taa_in = p64["out"].astype(np.float32)
    e = {"taa": R.rel_max(p32["out"], p64["out"]), "pass": R.rel_max(n32["out"], n64["out"]),
         "unsharpen": R.rel_max(T.unsharpen(taa_in, np.float32), T.unsharpen(taa_in, np.float64))}
    print(f"{w}x{h} e32 " + ", ".join(f"{k} {x:.2e}" for k, x in e.items()))
    for k, x in e.items():
        assert x <= 10 * E32_MEASURED[(w, h)][k], k


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_taa_pass_matches_restatement(core, w, h):
    b = make_buffers(w, h)
    p64, p32 = T.taa_pass(b["linear"], b["prev"], b["motion"], True, np.float64), T.taa_pass(b["linear"], b["prev"], b["motion"], True, np.float32)
    assert np.array_equal(p64["inside"], p32["inside"]) and np.array_equal(p64["fallback"], p32["fallback"])      # nothing to exclude
    e32 = R.rel_max(p32["out"][..., :3], p64["out"][..., :3])
    got = {}
    for lds in (1, 0):
        g = got[lds] = core.taa_unit(0, in_=b["linear"], prev=b["prev"], motion=b["motion"], history_valid=True, lds=bool(lds))
        err = R.rel_max(g[..., :3], p64["out"][..., :3])
        print(f"{w}x{h} taa pass lds {lds}: kernel {err:.2e}, e32 {e32:.2e}, bound {4 * e32:.2e}")
        assert np.array_equal(g[..., 3], np.zeros((h, w), np.float32))
        assert err <= 4 * e32
    assert R.rel_max(got[1][..., :3], got[0][..., :3]) <= 4 * e32


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_taa_pass_without_history_passes_through(core, w, h):
    b = make_buffers(w, h)
    want = np.fmin(10.0, np.sqrt(b["linear"][..., :3].astype(np.float64)))
    e32 = R.rel_max(T.taa_pass(b["linear"], b["prev"], b["motion"], False, np.float32)["out"][..., :3], want)
    for lds in (1, 0):
        g = core.taa_unit(0, in_=b["linear"], prev=b["prev"], motion=b["motion"], history_valid=False, lds=bool(lds))
        err = R.rel_max(g[..., :3], want)
        print(f"{w}x{h} taa pass without history lds {lds}: kernel {err:.2e}, e32 {e32:.2e}")
        assert np.array_equal(g[..., 3], np.zeros((h, w), np.float32))
        assert err <= 4 * e32


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_unsharpen_matches_restatement(core, w, h):
    b = make_buffers(w, h)
    taa_in = T.taa_pass(b["linear"], b["prev"], b["motion"], True, np.float64)["out"].astype(np.float32)
    u64, u32 = T.unsharpen(taa_in, np.float64), T.unsharpen(taa_in, np.float32)
    e32 = R.rel_max(u32[..., :3], u64[..., :3])
    g = core.taa_unit(1, in_=taa_in)
    err = R.rel_max(g[..., :3], u64[..., :3])
    print(f"{w}x{h} unsharpen: kernel {err:.2e}, e32 {e32:.2e}, bound {4 * e32:.2e}")
    assert np.array_equal(g[..., 3], np.ones((h, w), np.float32))
    assert err <= 4 * e32
