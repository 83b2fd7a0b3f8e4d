"""Sweep groups: with fewer hardware queues than streams the look-ahead path sweeps several submitted pairs in ONE diagonal
launch (vo_set_sweep_group / VO_SWEEP_GROUP).  What a pair computes must not depend on the group it travelled in: every
disparity, keypoint set, descriptor array and pose of a stream at group size 2, 3 and 4 equals the same stream with every pair
swept on its own, bit for bit."""
import numpy as np
import pytest

from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

N_PAIRS = 14            # not a multiple of 3 or 4: the last group of a burst is a partial one


@pytest.fixture(scope="module")
def c1():
    c = Corridor("C1")
    return c, c.pairs(10, N_PAIRS)


def _camera(c):
    return StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)


def _frame(odo, ok):
    k = odo.current_kps
    return (ok, odo.skip_cause, np.asarray(odo.current_disparity).copy(), k.xy.copy(), k.octave.copy(), k.angle.copy(),
            np.asarray(odo.current_desc).copy(), odo.c_T_w.copy())


def _same(a, b, what):
    assert a[:2] == b[:2], what
    for i, (x, y) in enumerate(zip(a[2:], b[2:])):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, i)


def _stream(cam, frames, lookahead, hook=None):
    """lookahead > 0: the staged stream through StereoOdometer.update with that many pairs started ahead; 0: every pair
    submitted from the host right before it is consumed (it is alone in the open group then) -> per-frame results"""
    cam.reset_lookahead()
    odo = StereoOdometer(cam, preprocessed_frames=True, rigidity_threshold=0.1, outlier_threshold=0.02)
    out = []
    if lookahead:
        cam.lookahead = lookahead
        staged = cam.stage_pairs(frames)
    for k, (L, R) in enumerate(frames):
        item = staged[k] if lookahead else cam.submit(L, R, preprocessed=True)
        if hook:
            hook(k, odo)
        out.append(_frame(odo, odo.update(item, None)))
    return out


def test_set_sweep_group_round_trip(c1):
    c, _ = c1
    ctx = _camera(c)._ctx
    engines = ctx.set_engines(0)
    auto = ctx.set_sweep_group(0)
    assert 1 <= auto <= min(engines, 12)
    for n in (1, 2, 3, 4, 6, 12):
        assert ctx.set_sweep_group(n) == min(n, engines) == ctx.set_sweep_group(0)
    assert ctx.set_sweep_group(10 ** 6) == min(12, engines)            # clamped to what one launch carries
    assert ctx.set_sweep_group(-5) == min(12, engines)                 # n <= 0 only asks
    ctx.set_engines(2)
    assert ctx.set_sweep_group(0) == 2                                 # an engine holds one member at a time
    ctx.set_engines(engines)
    assert ctx.lookahead_flush() == ctx.set_sweep_group(0)             # nothing open: a no-op that reports the size
    st = ctx.sweep_group_stats()
    assert st["open"] == 0 and st["full"] == st["consumer"] == st["flush"] == 0


@pytest.mark.parametrize("B", [2, 3, 4])
def test_stream_of_14_pairs_equals_the_ungrouped_stream(c1, B):
    """A burst (default look-ahead: the first update starts the thirteen other pairs -> full groups and a partial one closed
    by the flush) and a trickle (every pair submitted right before it is consumed: the consumer finds it alone in the open
    group) at group size B against the same two streams at group size 1; one pair of the burst against the oracle as well."""
    from oracle.odometer import RefStereoCamera
    c, frames = c1
    cam = _camera(c)
    ctx = cam._ctx
    default_la = cam.lookahead
    assert ctx.set_sweep_group(1) == 1
    want_burst, want_trickle = _stream(cam, frames, default_la), _stream(cam, frames, 0)
    st = ctx.sweep_group_stats()
    assert st["full"] == st["consumer"] == st["flush"] == st["other"] == 0 and st["open"] == 0    # B = 1 never defers
    assert ctx.set_sweep_group(B) == B
    seen = {"open": 0}

    def watch(k, odo):
        seen["open"] = max(seen["open"], ctx.sweep_group_stats()["open"])

    got_burst = _stream(cam, frames, default_la, watch)
    st = ctx.sweep_group_stats()
    assert st["full"] >= (N_PAIRS - 1) // B and st["flush"] >= 1 and st["open"] == 0, st           # 13 = q * B + a remainder of 1
    got_trickle = _stream(cam, frames, 0, watch)
    st = ctx.sweep_group_stats()
    assert st["consumer"] >= N_PAIRS // 2 and st["open"] == 0, st
    assert seen["open"] == 1                                            # (the trickle's pair waited in the open group)
    for k in range(N_PAIRS):
        _same(got_burst[k], want_burst[k], ("burst", B, k))
        _same(got_trickle[k], want_trickle[k], ("trickle", B, k))
    assert all(f[0] for f in got_burst[1:])                             # (poses really were estimated)
    rcam = RefStereoCamera(cam.Q, cam.valid_region_left, c.sgbm_params())
    k = 6
    rcam.compute_3d(*frames[k], preprocessed=True)
    vr = cam.valid_region_left
    assert np.array_equal(np.rint(got_burst[k][2] * 16).astype(np.int16), rcam.last_disp16[vr[1]:vr[3], vr[0]:vr[2]])
    assert ctx.sgbm_sweep_status() == 0


def test_reset_and_parameter_change_with_a_group_open(c1):
    """reset_lookahead() and vo_set_sgbm while a pair waits in the open group: the group is closed first (the pair finishes
    under the parameters it was submitted with), nothing stale is handed out afterwards."""
    c, frames = c1
    cam = _camera(c)
    ctx = cam._ctx
    ctx.set_sweep_group(1)
    want = _stream(cam, frames, 6)
    assert ctx.set_sweep_group(4) == 4
    opened = []

    def reset_mid_stream(k, odo):
        if k in (3, 6):
            opened.append(ctx.sweep_group_stats()["open"])
            odo.reset_lookahead()
            assert ctx.sweep_group_stats()["open"] == 0

    got = _stream(cam, frames, 6, reset_mid_stream)      # (the odometer polls the two oldest pairs ahead: the youngest stay grouped)
    assert opened and max(opened) >= 1, opened
    for k in range(N_PAIRS):
        _same(got[k], want[k], ("reset", k))
    # a parameter change: pair 1 waits in the open group when the parameters change; consumed afterwards it still is the
    # disparity of the parameters it was submitted under
    cam.reset_lookahead()
    staged = cam.stage_pairs(frames[:4])
    ctx.set_sgbm(c.sgbm_params())
    ctx.prefetch_staged_pair(5, 1, True)
    assert ctx.sweep_group_stats()["open"] == 1
    other = dict(c.sgbm_params(), P1=100, P2=1000)
    ctx.set_sgbm(other)
    st = ctx.sweep_group_stats()
    assert st["open"] == 0 and st["other"] >= 1
    shape = (c.h, c.w)
    d_old = ctx.download_disparity_f32(5, shape)
    ctx.set_sgbm(c.sgbm_params())
    ctx.load_staged_pair(6, 1, True)
    ctx.sgbm_compute(6)
    assert np.array_equal(d_old, ctx.download_disparity_f32(6, shape))
    ctx.set_sgbm(other)
    ctx.load_staged_pair(6, 1, True)
    ctx.sgbm_compute(6)
    assert not np.array_equal(d_old, ctx.download_disparity_f32(6, shape))
    ctx.lookahead_drop(5)
    del staged
