"""Host side of the dense direct alignment (no GPU): the constructor's keywords and the depth="sparse" refusal, the guard arithmetic
of StereoOdometer._direct on a stand-in context (every call bound against the real binding's signature), the binding's own checks,
and header / binding / library agreement on vo_direct_align."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("direct_refine", "direct_levels", "direct_iters", "direct_max_points", "direct_guard", "direct_status", "direct_record",
       "direct_accepted", "pose_information", "_direct_pair")


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_defaults_leave_the_object_as_it_was():
    sig = inspect.signature(StereoOdometer.__init__).parameters
    assert [sig[k].default for k in NEW[:5]] == [False, 3, 8, 16384, (0.1, 0.05)]
    for kw in (dict(), dict(direct_refine=False), dict(direct_refine=False, direct_levels=9, direct_guard="x"), dict(pose_method="pnp", depth="sparse")):
        o = StereoOdometer(_Cam(), **kw)
        assert not any(n in vars(o) for n in NEW), kw               # off: no new instance attribute, nothing validated
        assert o.direct_refine is False
    plain = set(vars(StereoOdometer(_Cam())))
    assert set(vars(StereoOdometer(_Cam(), direct_refine=True))) - plain == set(NEW)


def test_direct_keywords_are_validated():
    o = StereoOdometer(_Cam(), direct_refine=True, direct_levels=np.int64(2), direct_iters=5, direct_max_points=4096, direct_guard=[0.2, 0])
    assert (o.direct_levels, o.direct_iters, o.direct_max_points, o.direct_guard) == (2, 5, 4096, (0.2, 0.0))
    assert type(o.direct_levels) is int and type(o.direct_guard[1]) is float
    assert o.direct_status is None and o.direct_record is None and o.pose_information is None and o.direct_accepted is False
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="direct_refine must be"):
            StereoOdometer(_Cam(), direct_refine=bad)
    for kw in (dict(direct_levels=0), dict(direct_levels=5), dict(direct_levels=2.0), dict(direct_levels=True), dict(direct_iters=0),
               dict(direct_iters=21), dict(direct_iters="8"), dict(direct_max_points=0), dict(direct_max_points=1e4)):
        with pytest.raises(ValueError, match="direct_levels / direct_iters / direct_max_points"):
            StereoOdometer(_Cam(), direct_refine=True, **kw)
    for g in ((0.1,), (0.1, 0.05, 1), (-0.1, 0.05), (0.1, float("nan")), (float("inf"), 0.05), ("0.1", 0.05), (True, 0.05), 0.1, None):
        with pytest.raises(ValueError, match="direct_guard"):
            StereoOdometer(_Cam(), direct_refine=True, direct_guard=g)


def test_sparse_depth_is_refused():
    for kw in (dict(depth="sparse"), dict(depth="sparse", pose_method="pnp"), dict(depth="sparse", pose_method="pnp", track="map")):
        with pytest.raises(ValueError, match="direct_refine=True needs depth='dense'"):
            StereoOdometer(_Cam(), direct_refine=True, **kw)
    for kw in (dict(), dict(pose_method="pnp"), dict(match="klt"), dict(match="klt", pose_method="pnp", klt_fused=True)):
        StereoOdometer(_Cam(), direct_refine=True, **kw)


def test_binding_checks_its_parameters():
    P = _native.Context.direct_params
    assert P() == (3, 8, 16384, 8, 10.0, 4.0, 100.0, 0.1, 64)
    for kw in (dict(levels=0), dict(levels=5), dict(iters=21), dict(max_points=0), dict(grad_min=-1), dict(grad_min=256), dict(grad_min=8.0),
               dict(huber=0), dict(huber=float("nan")), dict(dmin=0), dict(dmin=5, dmax=4), dict(dmax=float("inf")), dict(z_min=-0.1),
               dict(min_pixels=5), dict(min_pixels=True)):
        with pytest.raises(ValueError):
            P(**kw)


# ---- the guard ---------------------------------------------------------------------------------------------------------------------
class _Ctx:
    """stands in for _native.Context: a scripted record, the call checked against the binding's signature"""

    def __init__(self, Rt, status=0):
        self.Rt, self.status, self.calls = np.asarray(Rt, np.float64), status, []

    def direct_align(self, *a, **kw):
        b = inspect.signature(_native.Context.direct_align).bind(None, *a, **kw)
        b.apply_defaults()
        self.calls.append({k: v for k, v in b.arguments.items() if k != "self"})
        return dict(status=self.status, iters_done=24, Rt=self.Rt, information=np.diag([1.0, 2, 3, 4, 5, 6]))


def _pose(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T


def _odo(Rt, status=0, skipped=0, pair=(3, 4), **kw):
    o = StereoOdometer(_Cam(), direct_refine=True, **kw)
    o._ctx, o._direct_pair, o.skipped_frames = _Ctx(Rt, status), pair, skipped
    return o


def test_the_call_carries_the_pair_the_pose_and_the_valid_disparity_range():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    o = _odo(T[:3], direct_levels=2, direct_iters=5, direct_max_points=4096)
    o._direct(T)
    (c,) = o._ctx.calls
    assert (c["slot_a"], c["slot_b"], c["levels"], c["iters"], c["max_points"]) == (3, 4, 2, 5, 4096)
    assert (c["dmin"], c["dmax"]) == (StereoOdometer.MIN_VALID_DISPARITY, StereoOdometer.MAX_VALID_DISPARITY)
    assert list(c["K4"]) == [400.0, 400.0, 320.0, 240.0] and np.array_equal(c["Rt0"], T[:3])


def test_guard_arithmetic():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    # inside both bounds: taken, with its information matrix
    near = _pose(0.01 + 0.04, (0.02, 0.0, 0.25 + 0.09))
    o = _odo(near[:3])
    out = o._direct(T)
    assert np.array_equal(out[:3], near[:3]) and np.array_equal(out[3], [0, 0, 0, 1])
    assert o.direct_accepted and o.direct_status == 0 and np.array_equal(o.pose_information, np.diag([1.0, 2, 3, 4, 5, 6]))
    # the motion D = T_refined T^-1 is what is bounded: past the metres, past the radians, each alone
    for moved in (_pose(0.0, (0.0, 0.0, 0.11)) @ T, _pose(0.06, (0, 0, 0)) @ T):
        o = _odo(moved[:3])
        assert o._direct(T) is T and not o.direct_accepted and o.direct_status == 0 and o.pose_information is None
    for moved in (_pose(0.0, (0.0, 0.0, 0.09)) @ T, _pose(0.04, (0, 0, 0)) @ T):
        o = _odo(moved[:3])
        assert o._direct(T) is not T and o.direct_accepted
    # a refusal never leaves the matrix of an older pose behind
    o = _odo(near[:3])
    o._direct(T)
    assert o.pose_information is not None
    o._ctx.Rt = (_pose(0.0, (0.0, 0.0, 0.11)) @ T)[:3]
    assert o._direct(T) is T and o.pose_information is None
    # scaled by the frames the pair spans, like the gates
    moved = _pose(0.0, (0.0, 0.0, 0.25)) @ T
    assert _odo(moved[:3], skipped=1)._direct(T) is T
    assert _odo(moved[:3], skipped=2)._direct(T) is not T
    # a status other than 0, or a pose that is not finite: the feature pose stands
    for status in (2, -1):
        o = _odo(near[:3], status=status)
        assert o._direct(T) is T and o.direct_status == status and not o.direct_accepted
    bad = near[:3].copy()
    bad[0, 3] = np.nan
    assert _odo(bad)._direct(T) is T
    # a guard of (0, 0) takes nothing but the feature pose itself
    assert _odo(near[:3], direct_guard=(0, 0))._direct(T) is T
    # frames that are not on the device cannot be aligned
    with pytest.raises(ValueError, match="device-resident"):
        _odo(near[:3], pair=None)._direct(T)


def test_the_gate_sees_the_refined_pose():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    far = _pose(0.0, (0.0, 0.0, 0.09)) @ T
    o = _odo(far[:3])
    o._ctx.rodrigues = lambda R: np.zeros(3)
    assert np.array_equal(o._gate(T), np.vstack([far[:3], [0, 0, 0, 1]]))
    assert o.direct_accepted and o.pose_information is not None
    gated = _odo((_pose(0.0, (0.0, 0.0, 0.09)) @ _pose(0.0, (0.0, 0.0, 0.95)))[:3])     # taken by the guard, refused by the distance gate
    gated._ctx.rodrigues = lambda R: np.zeros(3)
    assert gated._gate(_pose(0.0, (0.0, 0.0, 0.95))) is None and gated.skip_cause == "bigdist"
    assert gated.direct_accepted and gated.pose_information is None
    plain = StereoOdometer(_Cam())
    plain._ctx = _Ctx(far[:3])
    plain._ctx.rodrigues = lambda R: np.zeros(3)
    assert plain._gate(T) is T and not plain._ctx.calls


# ---- header, binding, library ------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_binding_agree():
    assert "vo_direct_align" in _native.SYMBOLS
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, "vo_direct_align")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo355.h")).read(), flags=re.S)
    decl = re.search(r"int\s+vo_direct_align\s*\(([^;]*)\)\s*;", txt).group(1)
    assert len(decl.split(",")) == len(_native.lib().vo_direct_align.argtypes) == 15
    assert int(re.search(r"#define\s+VO_DIRECT_MAX_LEVELS\s+(\d+)", txt).group(1)) == _native.DIRECT_MAX_LEVELS
    # the record: 16 + 4 x 32 + 96 + 216 + 16 bytes, as the header lays it out
    assert ctypes.sizeof(_native.DirectLevel) == 32 and ctypes.sizeof(_native.DirectRec) == 472
    rec = _native.DirectRec()
    rec.levels = 2
    rec.sums[1] = 5.0
    d = rec.as_dict()
    assert d["information"][0, 1] == d["information"][1, 0] == 5.0 and len(d["s"]) == 2 and d["Rt"].shape == (3, 4)
