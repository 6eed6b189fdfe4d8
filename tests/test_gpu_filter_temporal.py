"""The denoise mode over several frames (setting "filter"): history counts, motion vectors and history resets, on the
room at 96 x 54.

Still camera: every pixel's motion vector is its own position + 0.5 (within 1e-3 pixel: the reprojection runs in
float32), the history count of the pixels whose primary ray hits the same diffuse surface in every frame rises by 1 per
frame and stays at 15 (the sub-pixel jitter moves edges, and a specular chain's vertex changes with the random numbers).
Moved camera (a small translation, converge = Converge): the motion of the diffuse pixels is the restatement's analytic
reprojection through the previous view within 1e-3 pixel, and the pixels the restatement (float64 and float32 alike)
finds no history for have count 0.  converge = Restart resets every count."""
import numpy as np
import pytest

import filter_ref as R
from lighthouse2_amd import scene

pytestmark = pytest.mark.gpu

W, H = 96, 54
CONVERGE, RESTART = 0, 1


def _room(core):
    sc = scene.room_scene(20000, W, H)
    sc.load_into(core)
    core.set_target(W, H, 1)
    core.setting("filter", 1)
    return sc


def _moved(view, dx):
    v = type(view)()
    for name, _ in view._fields_:
        setattr(v, name, getattr(view, name))
    for name in ("pos", "p1", "p2", "p3"):
        p = getattr(view, name)
        setattr(v, name, type(p)(p.x + dx[0], p.y + dx[1], p.z + dx[2]))
    return v


def test_still_camera_history_counts(fresh_core):
    core = fresh_core
    sc = _room(core)
    ys, xs = np.mgrid[0:H, 0:W]
    stable, last = np.ones((H, W), bool), None
    for frame in range(18):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
        feat = core.filter_buffer("features")
        # the pixels whose primary ray hits the same diffuse surface in every frame so far (the sub-pixel jitter moves edges;
        # a specular chain's vertex depends on the frame's random numbers): the same material and a normal within the
        # history test's bound (dot >= 0.95; 0.96 here) of the previous frame's at that pixel, which is one of the taps
        hit = (feat[..., 2].view(np.float32) < 1e30) & (((feat[..., 3] >> 4) & 3) == 0)
        if last is not None:
            same = R.dot(R.unpack_normal(feat[..., 1], np.float64), R.unpack_normal(last[..., 1], np.float64)) >= 0.96
            hit &= same & ((feat[..., 3] >> 6) == (last[..., 3] >> 6)) & (((last[..., 3] >> 4) & 3) == 0)
        stable &= hit
        last = feat
        count = feat[..., 3] & 15
        assert stable.mean() > 0.3, (frame, stable.mean())
        assert np.array_equal(count[stable], np.full(int(stable.sum()), min(frame, 15), np.uint32)), frame
        if frame in (0, 1, 7, 17):
            motion = core.filter_buffer("motion")
            diffuse = ((feat[..., 3] >> 4) & 3) == 0
            assert np.abs(motion[..., 0] - (xs + 0.5)).max() <= 1e-3 and np.abs(motion[..., 1] - (ys + 0.5)).max() <= 1e-3, frame
    print(f"still camera: {stable.mean():.3f} of the pixels hit the same diffuse surface in all 18 frames")
    # a restart: no history again
    sc.render_frame(core, converge=RESTART)
    assert not (core.filter_buffer("features")[..., 3] & 15).any()
    sc.render_frame(core, converge=CONVERGE)
    feat2 = core.filter_buffer("features")
    assert np.array_equal((feat2[..., 3] & 15)[stable], np.ones(int(stable.sum()), np.uint32))


def test_moved_camera_reprojection(fresh_core):
    core = fresh_core
    sc = _room(core)
    for frame in range(3):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
    before = core.filter_buffer("features")[..., 3] & 15
    view2 = _moved(sc.view, (0.35, 0.1, -0.2))
    sc.render_frame(core, converge=CONVERGE, view=view2)
    feat, motion = core.filter_buffer("features"), core.filter_buffer("motion")
    bufs = dict(acc=core.filter_buffer("acc"), worldPos=core.filter_buffer("worldPos"), prevWorldPos=core.filter_buffer("prevWorldPos"),
                deltaDepth=core.filter_buffer("deltaDepth"), prevMoments=core.filter_buffer("prevMoments"))
    # the records as prepare saw them: the counts of the frame before (this frame's capture keeps them)
    seen = feat.copy()
    seen[..., 3] = (feat[..., 3] & ~np.uint32(15)) | before
    pv, cv = R.prev_view(R.view_tuple(sc.view), H), R.prev_view(R.view_tuple(view2), H)
    ref = {dt: R.prepare(bufs["acc"], seen, bufs["worldPos"], bufs["prevWorldPos"], bufs["deltaDepth"], bufs["prevMoments"], pv, cv, dt,
                         cam_stationary=True) for dt in (np.float64, np.float32)}
    diffuse = ((feat[..., 3] >> 4) & 3) == 0
    err = np.abs(motion[diffuse] - ref[np.float64]["motion"][diffuse]).max()
    moved = np.abs(motion[..., 0] - (np.mgrid[0:H, 0:W][1] + 0.5))[diffuse]
    print(f"moved camera: motion error {err:.2e} pixel over {int(diffuse.sum())} diffuse pixels; median shift {np.median(moved):.2f} pixel")
    assert np.median(moved) > 0.5                  # the camera did move
    assert err <= 1e-3
    lost = ~ref[np.float64]["found"] & ~ref[np.float32]["found"] & diffuse    # (specular pixels search for their history)
    kept = ref[np.float64]["found"] & ref[np.float32]["found"] & diffuse
    print(f"moved camera: {int(lost.sum())} pixels without history, {int(kept.sum())} with")
    assert lost.sum() > 20 and kept.sum() > 1000
    count = feat[..., 3] & 15
    assert not count[lost].any()
    assert np.array_equal(count[kept], np.minimum(before[kept] + 1, 15))
