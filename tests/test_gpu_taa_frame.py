"""The TAA stage of the denoise mode end to end (setting "TAA", applied while "filter" is): the setting and its buffers,
the times, the wiring of the two launches into the chain, and what the stage is for: the room at 128 x 72, 1 spp.
Every test first turns both settings on and reads "TAA" back as 1.

Wiring.  A restart frame, four more with the still camera, two with the camera translated: of each, the last pass's
output (phase3), the previous frame's TAA pixels, the motion vectors, this frame's TAA pixels and frame() are read back,
and the restatement (tests/taa_ref.py) of the two kernels on those inputs is compared with what the core wrote, at the unit
tests' bound (4 x e32 of these inputs: tests/test_gpu_taa_kernels.py).  The restart frame passes through, and a frame's
history is the previous frame's TAA pixels bit for bit.

Flicker.  Still camera, 24 frames, with TAA off and on: the per-pixel standard deviation of frame() over frames 16 .. 23,
averaged over the image and over the edge pixels (a material or normal change against a 4-neighbour in the features of any
of those frames), must both be lower with TAA; no factor is derivable.
Measured: image 0.1020 -> 0.0256 (x 3.99); edge pixels (0.665 of the image) 0.1443 -> 0.0335 (x 4.30).

Not worse than no filter.  As tests/test_gpu_filter_frame.py: frame 8's raw 1-spp image, its filtered frame and its TAA
frame against a 512-frame filter-off accumulation; the TAA frame's rel-L2 error must be below the raw image's.  (Whether
TAA beats the filter alone is not asked: it blends in gamma space and caps radiance where it has history.)
Measured: raw 0.8353, filtered 0.4374, filtered + TAA 0.3788."""
import os

import numpy as np
import pytest

import filter_ref as R
import taa_ref as T
from lighthouse2_amd import scene
from lighthouse2_amd.core import RenderCore

pytestmark = pytest.mark.gpu

W, H = 128, 72
CONVERGE, RESTART = 0, 1


def _rel(a, b):
    return float(np.linalg.norm(a[..., :3] - b[..., :3]) / np.linalg.norm(b[..., :3]))


def _taa_on(core):
    core.setting("filter", 1)
    core.setting("TAA", 1)
    assert core.get_setting("TAA") == 1


def _moved(view, dx):
    v = type(view)()
    for name, _ in view._fields_:
        setattr(v, name, getattr(view, name))
    for name in ("pos", "p1", "p2", "p3"):
        p = getattr(view, name)
        setattr(v, name, type(p)(p.x + dx[0], p.y + dx[1], p.z + dx[2]))
    return v


@pytest.fixture(scope="module")
def room_core():
    c = RenderCore(device=int(os.environ.get("LH2_TEST_DEVICE", "0")))
    sc = scene.room_scene(20000, W, H)
    sc.load_into(c)
    c.set_target(W, H, 1)
    yield c, sc
    c.close()


def test_default_is_off():
    c = RenderCore(device=int(os.environ.get("LH2_TEST_DEVICE", "0")))
    try:
        assert c.get_setting("TAA") == 0
        _taa_on(c)
    finally:
        c.close()


def test_settings_buffers_and_times(room_core):
    core, sc = room_core
    _taa_on(core)
    # TAA without the filter: not applied, the plain frame, no TAA times
    core.setting("filter", 0)
    core.setting("TAA", 0)
    sc.render_frame(core)
    plain = core.frame()
    core.setting("TAA", 1)
    assert core.get_setting("TAA") == 0
    sc.render_frame(core)
    assert _rel(core.frame(), plain) <= 1e-4
    assert not core.taa_times().any() and core.stats().filterTime == 0
    # the filter on: the kept wish applies
    core.setting("filter", 1)
    assert core.get_setting("filter") == 1 and core.get_setting("TAA") == 1
    sc.render_frame(core)
    sc.render_frame(core, converge=CONVERGE)
    st, kt, tt = core.stats(), core.filter_times(), core.taa_times()
    assert (tt > 0).all() and (kt > 0).all()
    print(f"filterTime {st.filterTime * 1e3:.4f} ms, kernels {kt} + {tt} ms, renderTime {st.renderTime * 1e3:.4f} ms")
    assert st.filterTime * 1e3 >= float(kt.sum() + tt.sum()) * (1 - 1e-5) and st.filterTime < st.renderTime
    assert core.filter_buffer("taa").shape == (H, W, 4) and core.filter_buffer("prevtaa").shape == (H, W, 4)
    # filter off and on again keeps the wish
    core.setting("filter", 0)
    assert core.get_setting("TAA") == 0
    with pytest.raises(Exception, match="filter"):
        core.filter_buffer("taa")
    core.setting("filter", 1)
    assert core.get_setting("TAA") == 1
    sc.render_frame(core)
    assert (core.taa_times() > 0).all()
    # TAA off: its buffers go, the filter stays, and the frame is the last pass's again
    core.setting("TAA", 0)
    assert core.get_setting("TAA") == 0 and core.get_setting("filter") == 1
    with pytest.raises(Exception, match="TAA"):
        core.filter_buffer("taa")
    sc.render_frame(core, converge=CONVERGE)
    assert not core.taa_times().any() and (core.filter_times() > 0).all()
    assert np.array_equal(core.filter_buffer("phase3"), core.frame())
    core.setting("filter", 0)


def test_toggle_keeps_the_filter_history(room_core):
    """Turning TAA on amid filtered frames drops only its own history: the history counts go on, the first TAA frame passes through."""
    core, sc = room_core
    _taa_on(core)
    core.setting("TAA", 0)
    for frame in range(3):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
    before = core.filter_buffer("features")[..., 3] & 15
    core.setting("TAA", 1)
    core.setting("TAA", 1)                                  # an unchanged value: nothing happens
    sc.render_frame(core, converge=CONVERGE)
    after = core.filter_buffer("features")[..., 3] & 15
    assert before.max() == 2 and after.max() == 3           # the filter's history went on
    lin, taa = core.filter_buffer("phase3"), core.filter_buffer("taa")
    assert np.array_equal(taa[..., :3], np.fmin(np.float32(10), np.sqrt(lin[..., :3])))      # no TAA history: passed through
    core.setting("TAA", 0)
    core.setting("filter", 0)


def test_two_devices_do_neither(fresh_core):
    core = fresh_core
    _taa_on(core)
    sc = scene.room_scene(20000, W, H)
    core.setting("deviceCount", 2)
    assert core.get_setting("filter") == 0 and core.get_setting("TAA") == 0
    sc.load_into(core)
    core.set_target(W, H, 1)
    sc.render_frame(core)
    multi = core.frame()
    assert core.stats().filterTime == 0
    core.setting("TAA", 1)                                  # asked for again: still not applied
    assert core.get_setting("TAA") == 0
    one = RenderCore(device=int(os.environ.get("LH2_TEST_DEVICE", "0")))
    try:
        sc.load_into(one)
        one.set_target(W, H, 1)
        sc.render_frame(one)
        assert _rel(multi, one.frame()) <= 1e-4
    finally:
        one.close()


def test_wiring_matches_restatement(room_core):
    core, sc = room_core
    _taa_on(core)
    views = [sc.view] * 5 + [_moved(sc.view, (0.35, 0.1, -0.2)), _moved(sc.view, (0.6, 0.15, -0.3))]
    last_taa = None
    for k, view in enumerate(views):
        sc.render_frame(core, converge=RESTART if k == 0 else CONVERGE, view=view)
        lin, prev, motion = core.filter_buffer("phase3"), core.filter_buffer("prevtaa"), core.filter_buffer("motion")
        taa, frame = core.filter_buffer("taa"), core.frame()
        if last_taa is not None:
            assert prev.tobytes() == last_taa.tobytes(), k                          # the history is the previous frame's TAA pixels
        last_taa = taa
        p64, p32 = T.taa_pass(lin, prev, motion, k > 0, np.float64), T.taa_pass(lin, prev, motion, k > 0, np.float32)
        assert np.array_equal(p64["inside"], p32["inside"]) and np.array_equal(p64["fallback"], p32["fallback"])
        if k == 0:
            assert not p64["inside"].any()
            assert np.array_equal(taa[..., :3], np.fmin(np.float32(10), np.sqrt(lin[..., :3])))    # the restart frame passes through
        else:
            assert p64["inside"].mean() > 0.5, k
        e32 = R.rel_max(p32["out"][..., :3], p64["out"][..., :3])
        err = R.rel_max(taa[..., :3], p64["out"][..., :3])
        u64, u32 = T.unsharpen(taa, np.float64), T.unsharpen(taa, np.float32)
        e32u, erru = R.rel_max(u32[..., :3], u64[..., :3]), R.rel_max(frame[..., :3], u64[..., :3])
        print(f"frame {k}: inside {p64['inside'].mean():.3f}; taa kernel {err:.2e}, e32 {e32:.2e}; unsharpen kernel {erru:.2e}, e32 {e32u:.2e}")
        assert not taa[..., 3].any() and np.array_equal(frame[..., 3], np.ones((H, W), np.float32))
        assert err <= 4 * e32, k
        assert erru <= 4 * e32u, k
    moved = np.abs(core.filter_buffer("motion")[..., 0] - (np.mgrid[0:H, 0:W][1] + 0.5))
    assert np.median(moved) > 0.5                                                   # the camera did move
    core.setting("TAA", 0)
    core.setting("filter", 0)


def _edges(feat):
    """Pixels whose material or normal differs from a 4-neighbour's."""
    mat = feat[..., 3] >> 6
    n = R.unpack_normal(feat[..., 1], np.float64)
    e = np.zeros(mat.shape, bool)
    for axis in (0, 1):
        a, b = [slice(None)] * 2, [slice(None)] * 2
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        d = (mat[a] != mat[b]) | (R.dot(n[a], n[b]) < 0.95)
        e[a] |= d
        e[b] |= d
    return e


def test_flicker_is_lower_with_taa(room_core):
    core, sc = room_core
    _taa_on(core)
    sd, edge = {}, np.zeros((H, W), bool)
    for taa in (0, 1):
        core.setting("TAA", taa)
        frames = []
        for k in range(24):
            sc.render_frame(core, converge=RESTART if k == 0 else CONVERGE)
            if k >= 16:
                frames.append(core.frame()[..., :3])
                edge |= _edges(core.filter_buffer("features"))
        sd[taa] = np.std(np.stack(frames), axis=0).mean(-1)
    core.setting("TAA", 0)
    core.setting("filter", 0)
    assert 0 < edge.mean() < 1
    whole, edges = (sd[0].mean(), sd[1].mean()), (sd[0][edge].mean(), sd[1][edge].mean())
    print(f"flicker (std over frames 16..23): image {whole[0]:.5f} -> {whole[1]:.5f} (x {whole[0] / whole[1]:.2f}), "
          f"edge pixels ({edge.mean():.3f} of the image) {edges[0]:.5f} -> {edges[1]:.5f} (x {edges[0] / edges[1]:.2f})")
    assert whole[1] < whole[0]
    assert edges[1] < edges[0]


def test_taa_frame_is_closer_to_the_converged_one_than_the_raw_one(room_core):
    core, sc = room_core
    _taa_on(core)
    core.setting("filter", 0)
    acc7 = None
    for frame in range(512):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
        if frame == 7:
            acc7 = core.accumulator()
        if frame == 8:
            raw = core.accumulator() - acc7
    converged = core.frame()
    core.setting("filter", 1)
    out = {}
    for taa in (0, 1):
        core.setting("TAA", taa)
        for frame in range(9):
            sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
        out[taa] = core.frame()
    core.setting("TAA", 0)
    core.setting("filter", 0)
    assert np.isfinite(out[1]).all()
    e_raw, e_filt, e_taa = _rel(raw, converged), _rel(out[0], converged), _rel(out[1], converged)
    print(f"rel-L2 against 512 frames: raw 1 spp {e_raw:.4f}, filtered {e_filt:.4f}, filtered + TAA {e_taa:.4f}")
    assert e_taa < e_raw
