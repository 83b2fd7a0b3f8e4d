"""Host side of the Lucas-Kanade front end (no GPU): the constructor's keywords, what StereoOdometer._pair_klt does with the tracks
(on a stand-in context, every call bound against the real binding's signature), and header / binding agreement on vo_klt_*."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native
from openvo_amd.features import DeviceImage, KeyPointList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("match", "klt_window", "klt_levels", "klt_fb", "klt_counts")


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_defaults_leave_the_object_as_it_was():
    sig = inspect.signature(StereoOdometer.__init__).parameters
    assert [sig[k].default for k in ("match", "klt_window", "klt_levels", "klt_fb")] == ["orb", 21, 4, 1.0]
    for kw in (dict(), dict(match="orb"), dict(match="orb", klt_window=9, klt_levels=2, klt_fb=0.5), dict(pose_method="pnp", depth="sparse")):
        o = StereoOdometer(_Cam(), **kw)
        assert not any(n in vars(o) for n in NEW), kw               # off: no new instance attribute
        assert o.match == "orb"
    plain = set(vars(StereoOdometer(_Cam())))
    assert set(vars(StereoOdometer(_Cam(), match="klt", pose_method="pnp"))) - plain == set(NEW)


def test_klt_keywords_are_validated():
    o = StereoOdometer(_Cam(), match="klt", klt_window=9, klt_levels=np.int64(2), klt_fb=0)
    assert (o.match, o.klt_window, o.klt_levels, o.klt_fb, o.klt_counts) == ("klt", 9, 2, 0.0, None)
    assert type(o.klt_window) is int and type(o.klt_levels) is int and type(o.klt_fb) is float
    for bad in ("KLT", "lk", None, 1, True, b"klt"):
        with pytest.raises(ValueError, match="match must be"):
            StereoOdometer(_Cam(), match=bad)
    for kw in (dict(klt_window=4), dict(klt_window=8), dict(klt_window=33), dict(klt_window=21.0), dict(klt_window=True), dict(klt_window="21"),
               dict(klt_levels=0), dict(klt_levels=7), dict(klt_levels=2.0), dict(klt_levels=None), dict(klt_fb=-1), dict(klt_fb=float("nan")),
               dict(klt_fb=float("inf")), dict(klt_fb="1"), dict(klt_fb=True)):
        for match in ("orb", "klt"):                                # (validated like the other keywords: whatever the mode)
            with pytest.raises(ValueError, match="klt_"):
                StereoOdometer(_Cam(), match=match, **kw)


def test_combinations_that_have_no_meaning_are_refused():
    with pytest.raises(ValueError, match="needs pose_method='pnp'"):
        StereoOdometer(_Cam(), match="klt", depth="sparse", pose_method="umeyama")
    StereoOdometer(_Cam(), match="klt", depth="sparse", pose_method="pnp")
    StereoOdometer(_Cam(), match="klt", depth="dense", pose_method="umeyama")
    with pytest.raises(ValueError, match="track"):
        StereoOdometer(_Cam(), match="klt", track="map", depth="sparse", pose_method="pnp")
    for kw in (dict(cross_check=True), dict(match_window=20), dict(match_window=(30, 10)),
               dict(loop_check=40, depth="sparse", pose_method="pnp")):
        with pytest.raises(ValueError, match="descriptor matcher"):
            StereoOdometer(_Cam(), match="klt", **kw)
        StereoOdometer(_Cam(), match="orb", **kw)


# ---- the pair step on a stand-in context ---------------------------------------------------------------------------------------------
def _bound(fn, *a, **kw):
    b = inspect.signature(getattr(_native.Context, fn)).bind(None, *a, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k != "self"}


class _Frame:
    live = True

    def __init__(self, slot, roi=(16, 8, 336, 248)):
        self.slot, self.roi = slot, roi


class _Ctx:
    """stands in for _native.Context: scripted tracks and lookups, every call checked against the binding's signature"""
    kp_cap = 2024

    def __init__(self, n=40, status=None, lookup_a=None, lookup_b=None, best=30):
        self.n, self.calls = n, []
        self.xy_a = np.stack([np.arange(n) * 5.0 + 20, np.arange(n) * 3.0 + 30], 1).astype(np.float32)
        self.xy_b = self.xy_a + np.float32(1.5)
        self.status = np.zeros(n, np.uint8) if status is None else np.asarray(status, np.uint8)
        self.lookup_a, self.lookup_b, self.best = lookup_a, lookup_b, best

    def klt_track(self, *a, **kw):
        self.calls.append(("klt_track", _bound("klt_track", *a, **kw)))
        return self.xy_b.copy(), self.status.copy(), np.full(self.n, 9, np.int32)

    def points3d_at(self, *a, **kw):
        b = _bound("points3d_at", *a, **kw)
        self.calls.append(("points3d_at", b))
        xy = np.asarray(b["xy"])
        x0, y0, x1, y1 = 16, 8, 336, 248
        assert ((xy >= 0).all() and (xy[:, 0] < x1 - x0).all() and (xy[:, 1] < y1 - y0).all())         # (the native call refuses anything else)
        pts = np.stack([xy[:, 0] * 0.01, xy[:, 1] * 0.01, np.full(len(xy), 5.0)], 1).astype(np.float32)
        st = np.zeros(len(xy), np.uint8)
        hook = self.lookup_a if b["slot"] == 3 else self.lookup_b
        if hook is not None:
            hook(xy, pts, st)
        return pts, st

    def ransac_pnp(self, *a, **kw):
        b = _bound("ransac_pnp", *a, **kw)
        self.calls.append(("ransac_pnp", b))
        Rt = np.hstack([np.eye(3), [[0.01], [0.0], [0.2]]])
        return dict(Rt=Rt, best_count=min(self.best, len(b["pts3d"])), best_iter=1, mask=np.ones(len(b["pts3d"]), np.uint8))

    def umeyama(self, src, dst, force_rotation=True):
        self.calls.append(("umeyama", dict(n=len(src))))
        return np.hstack([np.eye(3), [[0.0], [0.0], [0.1]]]), 1.0

    @staticmethod
    def rodrigues(R):
        return np.zeros(3)


def _odo(ctx, **kw):
    cam = _Cam()
    cam._ctx = ctx
    o = StereoOdometer(cam, match="klt", **kw)
    fa, fb = _Frame(3), _Frame(4)
    ka, kb = KeyPointList({"xy": ctx.xy_a}, frame=fa), KeyPointList({"xy": ctx.xy_b}, frame=fb)
    ka.desc, kb.desc = object(), object()
    return o, (ka, ka.desc, DeviceImage(fa, "xyz"), kb, kb.desc, DeviceImage(fb, "xyz"))


def test_pnp_arm_keeps_status_zero_and_adds_the_roi_origin():
    st = np.zeros(40, np.uint8)
    st[[1, 5, 6]] = (1, 2, 8)
    ctx = _Ctx(status=st)
    o, args = _odo(ctx, pose_method="pnp", klt_window=15, klt_levels=3, klt_fb=0.5)
    T = o._try_pair(*args)
    assert T is not None and T[2, 3] == 0.2 and o.klt_counts == (40, 37) and o.skip_cause == ""
    names = [c[0] for c in ctx.calls]
    assert names == ["klt_track", "points3d_at", "ransac_pnp"]
    k = ctx.calls[0][1]
    assert (k["slot_a"], k["slot_b"]) == (3, 4) and k["kw"] == dict(win=15, levels=3, fb=0.5)
    keep = np.nonzero(st == 0)[0]
    assert ctx.calls[1][1]["slot"] == 3 and np.array_equal(ctx.calls[1][1]["xy"], ctx.xy_a[keep])
    r = ctx.calls[2][1]
    assert np.array_equal(r["pts2d"], ctx.xy_b[keep] + np.array([16, 8], np.float32)) and len(r["pts3d"]) == 37
    assert (r["iters"], r["thr"], r["seed"]) == (256, 1.5, 4321)


def test_a_failed_lookup_drops_the_track_and_never_raises():
    def hook_a(xy, pts, st):
        st[0], st[1] = 2, 1                       # no usable tap / NaN: the keypoint paths raise ZeroDivisionError on 2
        pts[2, 1] = np.inf

    def hook_b(xy, pts, st):
        st[3] = 2
        pts[4, 0] = np.nan

    ctx = _Ctx(lookup_a=hook_a)
    o, args = _odo(ctx, pose_method="pnp")
    assert o._try_pair(*args) is not None and len(ctx.calls[2][1]["pts3d"]) == 37
    ctx = _Ctx(lookup_a=hook_a, lookup_b=hook_b)
    ctx.xy_b[10] = (-0.5, 40.0)                   # a track that left the crop (and stayed inside the image)
    ctx.xy_b[11] = (100.0, 240.0)
    o, args = _odo(ctx, pose_method="umeyama")
    assert o._try_pair(*args) is not None
    assert [c[0] for c in ctx.calls] == ["klt_track", "points3d_at", "points3d_at", "umeyama"]
    assert len(ctx.calls[2][1]["xy"]) == 35 and ctx.calls[2][1]["slot"] == 4 and ctx.calls[3][1]["n"] == 33


def test_decisions_in_the_order_of_the_composed_pnp_path():
    st = np.full(40, 8, np.uint8)
    st[:9] = 0
    ctx = _Ctx(status=st)
    o, args = _odo(ctx, pose_method="pnp")
    assert o._try_pair(*args) is None and o.skip_cause == "matches" and [c[0] for c in ctx.calls] == ["klt_track"]
    assert o.klt_counts == (40, 9)

    def all_bad(xy, pts, st_):
        st_[3:] = 2
    ctx = _Ctx(lookup_a=all_bad)
    o, args = _odo(ctx, pose_method="pnp")
    assert o._try_pair(*args) is None and o.skip_cause == "matches" and [c[0] for c in ctx.calls] == ["klt_track", "points3d_at"]
    ctx = _Ctx(best=9)
    o, args = _odo(ctx, pose_method="pnp")
    assert o._try_pair(*args) is None and o.skip_cause == "outlier"
    ctx = _Ctx()
    o, args = _odo(ctx, pose_method="pnp")
    o.MAX_DISTANCE_CHANGE = 0.1
    assert o._try_pair(*args) is None and o.skip_cause == "bigdist"
    ctx = _Ctx(lookup_b=all_bad)
    o, args = _odo(ctx, pose_method="umeyama")
    assert o._try_pair(*args) is None and o.skip_cause == "matches" and "umeyama" not in [c[0] for c in ctx.calls]


def test_frames_off_the_device_are_a_value_error_and_nothing_is_begun_ahead():
    ctx = _Ctx()
    o, args = _odo(ctx, pose_method="pnp")
    args[0].frame.slot = None
    _Frame.live = property(lambda self: self.slot is not None)
    try:
        with pytest.raises(ValueError, match="device-resident"):
            o._try_pair(*args)
    finally:
        _Frame.live = True
    assert ctx.calls == []
    o._start_next_pose()                          # (no step is begun ahead in this mode: nothing is asked of the camera or the context)
    assert ctx.calls == [] and o._specs == {}


# ---- header / binding ------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "vo355.h")).read()
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    lib = _native.lib()
    ctype = {"vo_ctx*": ctypes.c_void_p, "int": ctypes.c_int, "double": ctypes.c_double}
    for name in ("vo_klt_track_host", "vo_klt_track"):
        assert hasattr(L, name) and name in _native.SYMBOLS, name
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        want = []
        for arg in re.sub(r"/\*.*?\*/", "", m.group(1)).split(","):
            t = " ".join(arg.replace("*", "* ").split()[:-1]).replace(" *", "*").replace("const ", "")
            want.append(ctypes.c_void_p if t.endswith("*") else ctype[t])
        assert list(getattr(lib, name).argtypes) == want, name
    src = open(os.path.join(ROOT, "openvo_amd", "_native.py")).read()
    assert not re.search(r"L\.vo_klt_\w+\.argtypes", src)          # bound in the loop form, like the sparse and map entries
    for meth in ("klt_track", "klt_track_host", "klt_params"):
        assert callable(getattr(_native.Context, meth, None)), meth
    assert _native.Context.klt_params() == (21, 4, 30, 0.01, 1e-4, 1.0)
    for kw in (dict(win=6), dict(levels=0), dict(iters=101), dict(eps=-1.0), dict(min_eig=float("nan")), dict(fb=float("inf"))):
        with pytest.raises(ValueError):
            _native.Context.klt_params(**kw)
    assert "klt.hip" in open(os.path.join(ROOT, "openvo_amd", "csrc", "Makefile")).read()
