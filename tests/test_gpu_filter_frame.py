"""The denoise mode end to end (setting "filter"): the setting, CoreStats::filterTime, the filtered frame's quality, the
way back to the unfiltered frame, and the multi-device rule.

Quality: the room at 128 x 72, still camera.  The filtered frame() of frame 8 and the raw 1-spp image of the same frame
index with the filter off (the accumulator after frame 8 less the accumulator after frame 7) are both compared with a
512-frame filter-off accumulation; the filtered frame's rel-L2 error must be the lower one (a fixed factor is not
derivable).  Measured: raw 0.835, filtered 0.437, ratio 1.91."""
import numpy as np
import pytest

from lighthouse2_amd import scene
from lighthouse2_amd.core import RenderCore

pytestmark = pytest.mark.gpu

W, H = 128, 72
CONVERGE, RESTART = 0, 1


def _rel(a, b):
    return float(np.linalg.norm(a[..., :3] - b[..., :3]) / np.linalg.norm(b[..., :3]))


@pytest.fixture(scope="module")
def room_core():
    c = RenderCore(device=0)
    sc = scene.room_scene(20000, W, H)
    sc.load_into(c)
    c.set_target(W, H, 1)
    yield c, sc
    c.close()


def test_setting_round_trip_and_filter_time(room_core):
    core, sc = room_core
    assert core.get_setting("filter") == 0
    assert core.get_setting("clampDirect") == 2.5 and core.get_setting("clampIndirect") == 15.0
    sc.render_frame(core)
    assert core.stats().filterTime == 0
    core.setting("filter", 1)
    assert core.get_setting("filter") == 1
    sc.render_frame(core)
    st = core.stats()
    assert st.filterTime > 0 and st.filterTime < st.renderTime
    assert (core.filter_times() > 0).all()
    core.setting("clampIndirect", 8.0)
    assert core.get_setting("clampIndirect") == 8.0
    core.setting("clampIndirect", 15.0)
    core.setting("filter", 0)
    assert core.get_setting("filter") == 0
    sc.render_frame(core)
    assert core.stats().filterTime == 0


def test_filtered_frame_is_closer_to_the_converged_one(room_core):
    core, sc = room_core
    core.setting("filter", 0)
    # filter off: the raw sample of frame 8, then the 512-frame accumulation
    acc7 = None
    for frame in range(512):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
        if frame == 7:
            acc7 = core.accumulator()
        if frame == 8:
            raw = core.accumulator() - acc7
    converged = core.frame()
    core.setting("filter", 1)
    for frame in range(9):
        sc.render_frame(core, converge=RESTART if frame == 0 else CONVERGE)
    filtered = core.frame()
    planes = core.filter_buffer("acc")
    core.setting("filter", 0)
    # the same samples went in: the planes of frame 8 are the raw image of frame 8
    assert _rel(planes[0] + planes[1], raw) <= 1e-3
    assert np.isfinite(filtered).all()
    e_raw, e_filt = _rel(raw, converged), _rel(filtered, converged)
    print(f"rel-L2 against 512 frames: raw 1 spp {e_raw:.4f}, filtered {e_filt:.4f}, ratio {e_raw / e_filt:.2f}")
    assert e_filt < e_raw


def test_filter_off_again_is_the_unfiltered_frame(room_core):
    core, sc = room_core
    core.setting("filter", 0)
    sc.render_frame(core)
    ref = core.frame()
    core.setting("filter", 1)
    sc.render_frame(core)
    sc.render_frame(core, converge=CONVERGE)
    assert _rel(core.frame(), ref) > 1e-2              # the filtered frame is another image
    core.setting("filter", 0)
    sc.render_frame(core, converge=CONVERGE)           # the switch itself restarts the accumulation
    assert _rel(core.frame(), ref) <= 1e-4
    with pytest.raises(Exception, match="filter"):
        core.filter_buffer("features")                 # the buffers went with the mode


def test_two_devices_do_not_filter(fresh_core):
    core = fresh_core
    sc = scene.room_scene(20000, W, H)
    core.setting("filter", 1)
    core.setting("deviceCount", 2)
    assert core.get_setting("filter") == 0
    sc.load_into(core)
    core.set_target(W, H, 1)
    sc.render_frame(core)
    multi = core.frame()
    assert core.stats().filterTime == 0
    core.setting("filter", 1)                          # asked for again: still not applied
    assert core.get_setting("filter") == 0
    sc.render_frame(core)
    assert _rel(core.frame(), multi) <= 1e-4
    one = RenderCore(device=0)
    try:
        sc.load_into(one)
        one.set_target(W, H, 1)
        sc.render_frame(one)
        assert _rel(multi, one.frame()) <= 1e-4
    finally:
        one.close()
