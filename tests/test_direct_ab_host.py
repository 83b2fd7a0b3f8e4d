"""Host side of the dense direct alignment's affine brightness term (no GPU): the constructor's direct_affine keyword and its attribute
rules, StereoOdometer._direct on a stand-in context bound against the real binding's signature (the call carries affine=True, the
brightness and the marginalised information are taken over), the binding's own checks and its record, and header / binding /
library agreement on vo_direct_align_ab."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFFINE = ("direct_affine", "direct_brightness")


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])


# ---- the keyword -------------------------------------------------------------------------------------------------------------------
def test_default_is_off_and_ignored_without_direct_refine():
    assert inspect.signature(StereoOdometer.__init__).parameters["direct_affine"].default is False
    assert StereoOdometer.direct_affine is False and StereoOdometer.direct_brightness is None      # class attributes
    for kw in (dict(), dict(direct_affine=True), dict(direct_affine="yes"), dict(direct_affine=True, direct_iters=1),
               dict(direct_refine=False, direct_affine=3)):
        o = StereoOdometer(_Cam(), **kw)                # direct_refine off: not validated, like the other direct_* keywords
        assert not any(n in vars(o) for n in AFFINE) and o.direct_affine is False and o.direct_brightness is None and o.direct_refine is False


def test_attributes_are_set_on_the_instance_only_in_affine_mode():
    plain = StereoOdometer(_Cam(), direct_refine=True)
    off = StereoOdometer(_Cam(), direct_refine=True, direct_affine=False)
    assert set(vars(off)) == set(vars(plain)) and not any(n in vars(plain) for n in AFFINE)
    assert plain.direct_affine is False and plain.direct_brightness is None
    on = StereoOdometer(_Cam(), direct_refine=True, direct_affine=True)
    assert set(vars(on)) - set(vars(plain)) == set(AFFINE)
    assert on.direct_affine is True and on.direct_brightness is None and on.pose_information is None
    assert StereoOdometer(_Cam(), direct_refine=True, direct_affine=np.bool_(True)).direct_affine is True


def test_keyword_is_validated_with_direct_refine_on():
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="direct_affine must be"):
            StereoOdometer(_Cam(), direct_refine=True, direct_affine=bad)
    for n in (1, 2):
        with pytest.raises(ValueError, match="direct_affine=True needs direct_iters >= 3"):
            StereoOdometer(_Cam(), direct_refine=True, direct_affine=True, direct_iters=n)
        StereoOdometer(_Cam(), direct_refine=True, direct_iters=n)                  # the plain alignment keeps its range
    assert StereoOdometer(_Cam(), direct_refine=True, direct_affine=True, direct_iters=3).direct_iters == 3
    with pytest.raises(ValueError, match="direct_levels / direct_iters / direct_max_points"):
        StereoOdometer(_Cam(), direct_refine=True, direct_affine=True, direct_iters=21)


# ---- the call ----------------------------------------------------------------------------------------------------------------------
class _Ctx:
    """stands in for _native.Context: a scripted record, the call checked against the binding's signature"""

    def __init__(self, Rt, status=0, iters_done=24):
        self.Rt, self.status, self.iters_done, self.calls = np.asarray(Rt, np.float64), status, iters_done, []

    def direct_align(self, *a, **kw):
        b = inspect.signature(_native.Context.direct_align).bind(None, *a, **kw)
        b.apply_defaults()
        self.calls.append({k: v for k, v in b.arguments.items() if k != "self"})
        out = dict(status=self.status, iters_done=self.iters_done, Rt=self.Rt, information=np.diag([1.0, 2, 3, 4, 5, 6]))
        if b.arguments["affine"]:
            out.update(gain=1.25, offset=-3.5, unknowns=8 if self.iters_done >= 3 else 6, information_full=np.eye(8),
                       information=np.diag([0.5, 1, 1.5, 2, 2.5, 3]))
        return out


def _pose(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T


def _odo(Rt, status=0, iters_done=24, **kw):
    o = StereoOdometer(_Cam(), direct_refine=True, **kw)
    o._ctx, o._direct_pair, o.skipped_frames = _Ctx(Rt, status, iters_done), (3, 4), 0
    return o


def test_binding_signature_has_the_keyword_last_and_off():
    sig = inspect.signature(_native.Context.direct_align).parameters
    assert list(sig)[-1] == "affine" and sig["affine"].default is False
    assert list(inspect.signature(_native.Context.direct_params).parameters) == ["levels", "iters", "max_points", "grad_min", "huber", "dmin", "dmax",
                                                                                  "z_min", "min_pixels"]
    assert _native.Context.direct_params() == (3, 8, 16384, 8, 10.0, 4.0, 100.0, 0.1, 64)       # its signature and its 9-tuple are kept


def test_the_call_carries_affine_only_in_affine_mode():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    near = _pose(0.01 + 0.04, (0.02, 0.0, 0.25 + 0.09))
    o = _odo(near[:3])
    o._direct(T)
    assert o._ctx.calls[0]["affine"] is False and o.direct_brightness is None and "direct_brightness" not in vars(o)
    assert np.array_equal(o.pose_information, np.diag([1.0, 2, 3, 4, 5, 6]))
    a = _odo(near[:3], direct_affine=True, direct_levels=2, direct_iters=5, direct_max_points=4096)
    out = a._direct(T)
    (c,) = a._ctx.calls
    assert c["affine"] is True and (c["slot_a"], c["slot_b"], c["levels"], c["iters"], c["max_points"]) == (3, 4, 2, 5, 4096)
    assert (c["dmin"], c["dmax"]) == (StereoOdometer.MIN_VALID_DISPARITY, StereoOdometer.MAX_VALID_DISPARITY) and np.array_equal(c["Rt0"], T[:3])
    assert np.array_equal(out[:3], near[:3]) and a.direct_accepted and a.direct_status == 0
    assert a.direct_brightness == (1.25, -3.5)
    assert np.array_equal(a.pose_information, np.diag([0.5, 1, 1.5, 2, 2.5, 3]))       # the marginalised matrix of the record


def test_guard_and_status_handling_are_unchanged_and_the_brightness_follows_the_step():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    near = _pose(0.01 + 0.04, (0.02, 0.0, 0.25 + 0.09))
    # past the guard: the feature pose stands, no information; the brightness is the step's all the same
    far = _odo((_pose(0.0, (0.0, 0.0, 0.11)) @ T)[:3], direct_affine=True)
    assert far._direct(T) is T and not far.direct_accepted and far.pose_information is None and far.direct_brightness == (1.25, -3.5)
    # a status other than 0: the feature pose stands; a brightness only where a free iteration completed (the third is the first)
    for status, done, want in ((2, 7, (1.25, -3.5)), (-1, 2, None), (2, 0, None)):
        o = _odo(near[:3], status=status, iters_done=done, direct_affine=True)
        assert o._direct(T) is T and o.direct_status == status and not o.direct_accepted and o.direct_brightness == want
    # never the brightness of an older step
    o = _odo(near[:3], direct_affine=True)
    o._direct(T)
    assert o.direct_brightness is not None
    o._ctx.status, o._ctx.iters_done = -1, 1
    assert o._direct(T) is T and o.direct_brightness is None and o.pose_information is None
    # the gates see the refined pose, as without the keyword
    g = _odo((_pose(0.0, (0.0, 0.0, 0.09)) @ T)[:3], direct_affine=True)
    g._ctx.rodrigues = lambda R: np.zeros(3)
    assert np.array_equal(g._gate(T)[:3], (_pose(0.0, (0.0, 0.0, 0.09)) @ T)[:3]) and g.direct_accepted


def test_binding_refuses_fewer_than_three_iterations_before_the_library():
    class _NoLib:
        _lib = type("L", (), {"vo_direct_align": None, "vo_direct_align_ab": None})()
        direct_params = staticmethod(_native.Context.direct_params)
    for n in (1, 2):
        with pytest.raises(ValueError, match="3 .. 20"):
            _native.Context.direct_align(_NoLib(), 0, 1, (1.0, 1.0, 0.0, 0.0), iters=n, affine=True)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="affine must be"):
            _native.Context.direct_align(_NoLib(), 0, 1, (1.0, 1.0, 0.0, 0.0), affine=bad)


# ---- header, binding, library ------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_binding_agree():
    assert "vo_direct_align_ab" in _native.SYMBOLS
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, "vo_direct_align_ab")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo355.h")).read(), flags=re.S)
    decl = re.search(r"int\s+vo_direct_align_ab\s*\(([^;]*)\)\s*;", txt).group(1)
    plain = re.search(r"int\s+vo_direct_align\s*\(([^;]*)\)\s*;", txt).group(1)
    assert len(decl.split(",")) == len(_native.lib().vo_direct_align_ab.argtypes) == 15
    assert decl.replace("vo_direct_ab_rec", "vo_direct_rec").split() == plain.split()        # the plain entry's arguments, the other record
    assert list(_native.lib().vo_direct_align_ab.argtypes) == list(_native.lib().vo_direct_align.argtypes)
    # the record as the header lays it out: 16 + 4 x 32 + 96 + 16 + 352 + 16 bytes; the plain record keeps its 472
    body = re.search(r"typedef\s+struct\s+vo_direct_ab_rec\s*\{(.*?)\}\s*vo_direct_ab_rec\s*;", txt, flags=re.S).group(1)
    names = [n.strip().split("[")[0] for decl_ in body.split(";") if decl_.strip() for n in decl_.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _native.DirectAbRec._fields_]
    assert ctypes.sizeof(_native.DirectAbRec) == 624 and ctypes.sizeof(_native.DirectRec) == 472
    assert _native.DirectAbRec.sums.size == 44 * 8 and _native.DirectAbRec.k.offset == 16 + 4 * 32 + 96


def test_record_as_dict():
    rec = _native.DirectAbRec()
    rec.levels, rec.unknowns, rec.k, rec.m = 2, 8, 1.5, -2.0
    H = np.diag([4.0, 4, 4, 4, 4, 4, 2, 1])
    H[0, 6] = H[6, 0] = 1.0
    H[6, 7] = H[7, 6] = 0.5
    rec.sums[:36] = list(H[np.triu_indices(8)])
    rec.sums[36:44] = list(range(1, 9))
    d = rec.as_dict()
    assert d["gain"] == 1.5 and d["offset"] == -2.0 and d["unknowns"] == 8 and len(d["s"]) == 2 and d["Rt"].shape == (3, 4)
    assert np.array_equal(d["information_full"], H) and d["sums"].shape == (44,) and np.array_equal(d["g"], np.arange(1.0, 9.0))
    want = np.linalg.inv(np.linalg.inv(H)[:6, :6])
    assert np.abs(d["information"] - want).max() <= 1e-12 and d["information"][0, 0] < 4.0 and np.array_equal(d["information"], d["information"].T)
    rec.unknowns = 6
    rec.sums[:] = [0.0] * 44
    rec.sums[1] = 5.0
    rec.sums[21] = 7.0
    d = rec.as_dict()
    assert d["information"][0, 1] == d["information"][1, 0] == 5.0 and np.array_equal(d["information"], d["information_full"][:6, :6])
    assert not d["information_full"][6:].any() and d["g"][0] == 7.0 and not d["g"][6:].any()
    rec.unknowns = 7
    with pytest.raises(ValueError):
        rec.as_dict()
