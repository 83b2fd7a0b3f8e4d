"""The Lucas-Kanade kernels (openvo_amd/csrc/klt.hip) held to the numpy restatement (tests/klt_ref.py) BIT FOR BIT: positions,
status bytes and iteration counts of every point, no tolerance and no point left out.  The restatement itself is held to what a
tracker must do in tests/test_klt_ref.py, on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from openvo_amd import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_cases as C                      # noqa: E402
import klt_ref as K                        # noqa: E402

pytestmark = pytest.mark.gpu

VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 320, 240, 32, 400)
    yield c
    c.close()


def _pairs(w, h):
    return (("smooth", C.smooth_pair(w, h)), ("corridor", C.corridor_pair(w, h)))


_REF = {}


def _ref(tex, w, h, win, levels, n, **kw):
    """the restatement's answer, computed once per case and shared"""
    key = (tex, w, h, win, levels, n, tuple(sorted(kw.items())))
    if key not in _REF:
        a, b = dict(_pairs(w, h))[tex]
        xy = C.points(w, h, n, extra=C.fixture()[2] if (w, h) == (160, 120) else ())
        _REF[key] = (a, b, xy, K.track(a, b, xy, win=win, levels=levels, **kw))
        for v in _REF[key][3]:
            v.setflags(write=False)
    return _REF[key]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("xy", "status", "iters")):
        if not C.same_bits(g, w):
            bad = np.nonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d points, first %d: %r != %r" % (what, name, len(bad), len(g), bad[0], g[bad[0]], w[bad[0]]))


@pytest.mark.parametrize("fb", (0.0, 1.0))
@pytest.mark.parametrize("w,h,win,levels", C.SHAPES)
def test_host_entry_equals_the_restatement_bit_for_bit(ctx, w, h, win, levels, fb):
    """every shape, both textures, 257 points: sub-pixel inputs, points within 2 px of every border and corner and beyond them,
    the flat patch, NaN and inf, far-away points, the fixture's oscillating points"""
    for tex, _ in _pairs(w, h):
        a, b, xy, want = _ref(tex, w, h, win, levels, 257, fb=fb)
        got = ctx.klt_track_host(a, b, xy, win=win, levels=levels, fb=fb)
        _same(got, want, "%s %dx%d win %d levels %d fb %g" % (tex, w, h, win, levels, fb))
        st = want[1]
        assert (st == 0).sum() >= 50 and ((st & 1).any() or tex == "corridor")      # (a real case: tracked points and a flat one)
        assert (st & 2).any() and (st == 4).sum() == 3
        if fb > 0:
            assert (st & 8).any()


@pytest.mark.parametrize("n", C.COUNTS)
def test_point_counts_around_a_workgroup(ctx, n):
    """n = 0, 1, one short of a workgroup's points, exactly that, one more, 257"""
    w, h, win, levels = C.SHAPES[0]
    a, b, xy, want = _ref("smooth", w, h, win, levels, n, fb=1.0)
    got = ctx.klt_track_host(a, b, xy, win=win, levels=levels, fb=1.0)
    assert len(got[0]) == n
    _same(got, want, "n = %d" % n)


def test_iteration_limit_and_oscillation_stop(ctx):
    """iters = 2: most points run to the limit on every level (the count says so); the fixture's points end a level by the
    oscillation stop under their parameters"""
    w, h, win, levels = C.SHAPES[2]
    a, b, xy, want = _ref("corridor", w, h, win, levels, 257, fb=0.0, iters=2)
    _same(ctx.klt_track_host(a, b, xy, win=win, levels=levels, fb=0.0, iters=2), want, "iters = 2")
    assert (want[2][want[1] == 0] == 2 * levels).sum() >= 20
    a, b, osc = C.fixture()
    tr = {}
    want = K.track(a, b, osc, fb=0.0, trace=tr, **C.OSC_PARAMS)
    assert len(osc) >= 4 and (tr["osc"] > 0).all() and (want[1] == 0).all()
    _same(ctx.klt_track_host(a, b, osc, fb=0.0, **C.OSC_PARAMS), want, "oscillation")
    # the corridor is where the counts vary
    a, b, xy, want = _ref("corridor", w, h, win, levels, 257, fb=0.0)
    ok = want[1] == 0
    assert want[2][ok].min() <= 12 and want[2][ok].max() >= 40


def test_every_window_size_and_level_count(ctx):
    """each kernel instantiation (windows 5 .. 31) and 1 .. 6 levels, 40 points each"""
    w, h = 160, 120
    a, b = C.corridor_pair(w, h)
    xy = C.points(w, h, 40)
    for win, levels in ((5, 6), (7, 1), (11, 2), (13, 4), (15, 3), (17, 2), (19, 5), (23, 2), (25, 3), (27, 2), (29, 2), (31, 4)):
        want = K.track(a, b, xy, win=win, levels=levels, fb=1.0)
        _same(ctx.klt_track_host(a, b, xy, win=win, levels=levels, fb=1.0), want, "win %d levels %d" % (win, levels))


def test_refusals_leave_the_outputs_untouched(ctx):
    lib, h = ctx._lib, ctx._h
    w, hh = 96, 64
    a, b = C.smooth_pair(w, hh)
    xy = C.points(w, hh, 8)
    p = _native._p

    def call(A=a, B=b, W=w, H=hh, XY=xy, n=8, win=9, levels=2, iters=30, eps=0.01, me=1e-4, fb=1.0, outs=(True, True, True), handle=h):
        o = (np.full((8, 2), -7.0, np.float32), np.full(8, 0xEE, np.uint8), np.full(8, -9, np.int32))
        args = [p(v) if keep else None for v, keep in zip(o, outs)]
        rc = lib.vo_klt_track_host(handle, None if A is None else p(A), None if B is None else p(B), W, H, None if XY is None else p(XY), n,
                                   win, levels, iters, eps, me, fb, *args)
        assert (o[0] == -7.0).all() and (o[1] == 0xEE).all() and (o[2] == -9).all() or rc == 0
        return rc

    assert call() == 0
    for kw in (dict(win=4), dict(win=8), dict(win=33), dict(win=3), dict(levels=0), dict(levels=7), dict(iters=0), dict(iters=101),
               dict(eps=-1.0), dict(eps=float("nan")), dict(me=float("inf")), dict(me=-1e-9), dict(fb=-0.5), dict(fb=float("nan")),
               dict(A=None), dict(B=None), dict(XY=None), dict(W=0), dict(H=-1), dict(n=-1), dict(outs=(False, True, True)),
               dict(outs=(True, False, True)), dict(outs=(True, True, False)), dict(handle=None)):
        assert call(**kw) == VO_E_ARG, kw
    assert call(W=ctx.max_w + 1) == VO_E_CAP and call(H=ctx.max_h + 1) == VO_E_CAP
    assert call(n=ctx.kp_cap + 1) == VO_E_CAP
    assert call(n=0, XY=None, outs=(False, False, False)) == 0          # n = 0 is valid and needs no array
    for kw in (dict(win=6), dict(levels=9), dict(fb=-1)):
        with pytest.raises(ValueError):
            ctx.klt_track_host(a, b, xy, **kw)
    with pytest.raises(ValueError):
        ctx.klt_track_host(a, b[:-1], xy)
    # and the context still works
    got = ctx.klt_track_host(a, b, xy, win=9, levels=2)
    _same(got, K.track(a, b, xy, win=9, levels=2), "after the refusals")


# ---- the slot entry ----------------------------------------------------------------------------------------------------------------------
def test_slot_entry_with_a_roi_equals_the_restatement_on_the_downloads(ctx):
    """two uploaded slots, a non-zero ROI: slot a's keypoints (crop pixels) against the restatement on the downloaded left images
    and keypoints with the ROI origin, bit for bit; and the refusals of the entry"""
    a, b, _ = C.fixture()
    h, w = a.shape
    roi = (9, 5, 152, 114)
    ctx.set_roi(*roi)
    try:
        ctx.upload_pair(0, a, a, True)
        ctx.upload_pair(1, b, b, True)
        lib, hd, p = ctx._lib, ctx._h, _native._p
        o = (np.full((ctx.kp_cap, 2), -7.0, np.float32), np.full(ctx.kp_cap, 0xEE, np.uint8), np.full(ctx.kp_cap, -9, np.int32))
        n = ctypes.c_int(-5)

        def call(sa=0, sb=1, win=21, levels=3, cap=ctx.kp_cap, outs=(True, True, True), n_out=True):
            args = [p(v) if keep else None for v, keep in zip(o, outs)]
            rc = lib.vo_klt_track(hd, sa, sb, win, levels, 30, 0.01, 1e-4, 1.0, *args, cap, ctypes.byref(n) if n_out else None)
            if rc != 0:
                assert (o[0] == -7.0).all() and (o[1] == 0xEE).all() and (o[2] == -9).all() and n.value == -5
            return rc

        assert call() == VO_E_STATE                                   # no keypoints in slot a yet
        kp = ctx.orb_slot(0, 200, 0)
        nk = len(kp["xy"])
        assert nk >= 20
        assert call(sb=2) == VO_E_STATE                               # no pair in slot b
        assert call(sa=-1) == VO_E_ARG and call(sb=_native.VO_NUM_SLOTS) == VO_E_ARG and call(win=22) == VO_E_ARG and call(levels=0) == VO_E_ARG
        assert call(outs=(False, True, True)) == VO_E_ARG and call(outs=(True, False, True)) == VO_E_ARG and call(n_out=False) == VO_E_ARG
        assert call(cap=nk - 1) == VO_E_CAP
        ctx.upload_pair(2, b[:-8], b[:-8], True)
        assert call(sb=2) == VO_E_STATE                               # shapes differ
        la, lb = ctx.download_left(0, (h, w)), ctx.download_left(1, (h, w))
        assert np.array_equal(la, a) and np.array_equal(lb, b)
        xy = ctx.download_keypoints(0)["xy"]
        for kw in (dict(win=21, levels=3, fb=1.0), dict(win=9, levels=2, fb=0.0)):
            want = K.track(la, lb, xy, origin=roi[:2], **kw)
            _same(ctx.klt_track(0, 1, **kw), want, "slots, %r" % (kw,))
            assert (want[1] == 0).sum() >= 10
        # a slot tracked into itself stays where it is, and iters_out may be NULL
        assert call(sb=0, outs=(True, True, False)) == 0 and n.value == nk
        assert C.same_bits(o[0][:nk], xy) and (o[1][:nk] == 0).all() and (o[2] == -9).all()
    finally:
        ctx.set_roi(0, 0, ctx.max_w, ctx.max_h)


# ---- the odometer --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(oracle):
    """corridor C1, the 12 pairs of the composed-path odometer test, and per frame what the CPU chain needs, taken from the device"""
    from openvo_amd import StereoCamera, StereoOdometer
    from openvo_amd.synth import Corridor
    cx = _native.Context(0, 640, 480, 64, 500)
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=cx)
    pairs = c.pairs(0, 12)
    probe = StereoOdometer(cam, preprocessed_frames=True)
    frames = []
    for L, R in pairs:
        x3, disp, left = cam.compute_3d(L, R, preprocessed=True)
        kps, _ = probe.orb.detectAndCompute(left, probe.feature_mask(disp))
        f = x3.frame
        frames.append(dict(left=f.full("left").copy(), xy=kps.xy.copy(), disp16=np.rint(f.full("disp") * 16).astype(np.int16)))
        del x3, disp, left, kps, f
    del probe
    yield dict(ctx=cx, cam=cam, pairs=pairs, frames=frames, tracks={}, oracle=oracle)
    cx.close()


@pytest.mark.parametrize("pose_method", ("pnp", "umeyama"))
def test_odometer_equals_the_cpu_chain(rig, pose_method):
    """StereoOdometer(match="klt") frame by frame against the restatement's tracks + the oracle's RANSAC PnP / Umeyama in the reference
    state machine: decisions, skip_cause and counts exactly, c_T_w to 1e-9"""
    import klt_chain_ref as KC
    from openvo_amd import StereoOdometer
    cam = rig["cam"]
    klt = dict(win=21, levels=4, fb=1.0)
    chain = KC.KltDenseChain(rig["oracle"], cam.Q, cam.valid_region_left, pose_method, klt)
    chain.tracks = rig["tracks"]                                      # (the two arms track the same pairs: computed once)
    odo = StereoOdometer(cam, preprocessed_frames=True, match="klt", pose_method=pose_method)
    for k, ((L, R), f) in enumerate(zip(rig["pairs"], rig["frames"])):
        got, want = odo.update(L, R), chain.update(f)
        assert got == want and odo.skip_cause == chain.skip_cause and odo.skipped_frames == chain.skipped_frames, k
        assert odo.klt_counts == chain.counts, k
        assert np.abs(odo.c_T_w - chain.c_T_w).max() <= 1e-9, k
        print("%s frame %2d: accepted %s cause %r tracks %s" % (pose_method, k, got, odo.skip_cause, odo.klt_counts))
    assert odo.klt_counts[1] >= 100 and not odo._specs
    assert np.linalg.norm(odo.c_T_w[:3, 3]) > 1.0                    # (it moved: 11 pairs of 0.25 m)


def test_run_with_lookahead_equals_update(rig):
    from openvo_amd import StereoOdometer
    cam = rig["cam"]
    a = StereoOdometer(cam, preprocessed_frames=True, match="klt", pose_method="pnp")
    want = [(a.update(L, R), a.skip_cause, a.c_T_w.copy()) for L, R in rig["pairs"][:6]]
    b = StereoOdometer(cam, preprocessed_frames=True, match="klt", pose_method="pnp")
    got = [(ok, b.skip_cause, b.c_T_w.copy()) for ok in b.run(iter(rig["pairs"][:6]))]
    assert len(got) == len(want) and not b._specs
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2])
    b.reset_lookahead()


def test_an_orb_odometer_is_unchanged_by_a_klt_odometer_on_the_same_context(rig):
    from openvo_amd import StereoOdometer
    cam, pairs = rig["cam"], rig["pairs"][:5]

    def orb_poses():
        o = StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp")
        out = [(o.update(L, R), o.skip_cause, o.c_T_w.copy()) for L, R in pairs]
        o.reset_lookahead()
        return out

    before = orb_poses()
    k = StereoOdometer(cam, preprocessed_frames=True, match="klt", pose_method="umeyama")
    used = [k.update(L, R) for L, R in pairs]
    assert used[0] and any(used[1:]) and k.klt_counts[1] >= 100        # (it tracked and placed frames; what it decides is held to the chain above)
    after = orb_poses()
    assert all(b[0] for b in before)
    for b, a in zip(before, after):
        assert b[0] == a[0] and b[1] == a[1] and np.array_equal(b[2], a[2])


def test_sparse_depth_arm_equals_its_cpu_chain(rig):
    """depth="sparse": the 3-D points are the per-keypoint cloud.  C1 frames 0 - 7 against the chain DESIGN 4k's figures come from
    (oracle ORB on both images, the restated sparse association, the restatement's tracks, the oracle's RANSAC)."""
    import klt_chain_ref as KC
    from openvo_amd import StereoOdometer
    from openvo_amd.synth import Corridor
    cam, pairs = rig["cam"], rig["pairs"][:8]
    ref = KC.KltSparseRefOdometer(rig["oracle"], cam.Q, cam.valid_region_left, nfeatures=500, klt=dict(win=21, levels=4, fb=1.0))
    odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", pose_method="pnp", match="klt")
    for k, (L, R) in enumerate(pairs):
        got, want = odo.update(L, R), ref.update(L, R)
        assert got == want and odo.skip_cause == ref.skip_cause, k
        if k:
            assert odo.klt_counts == ref.kept[-1], k
        assert np.abs(odo.c_T_w - ref.c_T_w).max() <= 1e-9, k
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(7)
    err = float(np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3]))
    print("sparse + klt + pnp, C1 frames 0 - 7: end point %.4f m off the ground truth" % err)
    assert err < 1.303
