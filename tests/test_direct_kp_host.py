"""Host side of the patch alignment (no GPU): the constructor's keywords and refusals, the guard arithmetic of StereoOdometer._patch on
a stand-in context (every call bound against the real binding's signature), the binding's own checks, and header / binding / library
agreement on vo_direct_align_kp."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = ("patch_refine", "patch_size", "patch_levels", "patch_iters", "patch_guard")
NEW = KEYWORDS + ("patch_status", "patch_record", "patch_accepted", "pose_information", "_patch_pair")
SPARSE = dict(depth="sparse", pose_method="pnp")


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_defaults_leave_the_object_as_it_was():
    sig = inspect.signature(StereoOdometer.__init__).parameters
    assert [sig[k].default for k in KEYWORDS] == [False, 5, 3, 4, (0.1, 0.05)]
    for kw in (dict(), dict(patch_refine=False), dict(patch_refine=False, patch_size=4, patch_levels=9, patch_guard="x"), SPARSE,
               dict(SPARSE, track="map"), dict(direct_refine=True)):
        o = StereoOdometer(_Cam(), **kw)
        assert not any(n in vars(o) for n in NEW if n != "pose_information" or not kw.get("direct_refine")), kw      # off: nothing added, nothing validated
        assert o.patch_refine is False
    plain = set(vars(StereoOdometer(_Cam(), **SPARSE)))
    assert set(vars(StereoOdometer(_Cam(), patch_refine=True, **SPARSE))) - plain == set(NEW)


def test_patch_keywords_are_validated():
    o = StereoOdometer(_Cam(), patch_refine=True, patch_size=np.int64(7), patch_levels=2, patch_iters=6, patch_guard=[0.2, 0], **SPARSE)
    assert (o.patch_size, o.patch_levels, o.patch_iters, o.patch_guard) == (7, 2, 6, (0.2, 0.0))
    assert type(o.patch_size) is int and type(o.patch_guard[1]) is float
    assert o.patch_status is None and o.patch_record is None and o.pose_information is None and o.patch_accepted is False
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="patch_refine must be"):
            StereoOdometer(_Cam(), patch_refine=bad, **SPARSE)
    for kw in (dict(patch_size=4), dict(patch_size=1), dict(patch_size=9), dict(patch_size=5.0), dict(patch_size=True), dict(patch_levels=0),
               dict(patch_levels=5), dict(patch_levels=2.0), dict(patch_iters=0), dict(patch_iters=21), dict(patch_iters="4")):
        with pytest.raises(ValueError, match="patch_levels / patch_iters / patch_size"):
            StereoOdometer(_Cam(), patch_refine=True, **dict(SPARSE, **kw))
    for g in ((0.1,), (0.1, 0.05, 1), (-0.1, 0.05), (0.1, float("nan")), (float("inf"), 0.05), ("0.1", 0.05), (True, 0.05), 0.1, None):
        with pytest.raises(ValueError, match="patch_guard"):
            StereoOdometer(_Cam(), patch_refine=True, patch_guard=g, **SPARSE)


def test_constructor_rules():
    for kw in (dict(), dict(pose_method="pnp"), dict(depth="dense", match="klt")):
        with pytest.raises(ValueError, match="patch_refine=True needs depth='sparse'"):
            StereoOdometer(_Cam(), patch_refine=True, **kw)
    with pytest.raises(ValueError, match="patch_refine=True needs track='pair'"):
        StereoOdometer(_Cam(), patch_refine=True, track="map", **SPARSE)
    with pytest.raises(ValueError, match="direct_refine=True needs depth='dense'"):         # the existing message stays
        StereoOdometer(_Cam(), patch_refine=True, direct_refine=True, **SPARSE)
    with pytest.raises(ValueError, match="direct_refine=True needs depth='dense'"):
        StereoOdometer(_Cam(), direct_refine=True, **SPARSE)
    # both pose methods; match="orb" and "klt" where those accept sparse depth, klt_fused included
    for kw in (dict(depth="sparse"), SPARSE, dict(SPARSE, cross_check=True, match_window=(24, 16)), dict(SPARSE, match="klt"),
               dict(SPARSE, match="klt", klt_fused=True), dict(SPARSE, pnp_refine=3, pnp_lo_rounds=2)):
        assert StereoOdometer(_Cam(), patch_refine=True, **kw).patch_refine is True
    with pytest.raises(ValueError, match="match='klt' with depth='sparse' needs pose_method='pnp'"):
        StereoOdometer(_Cam(), patch_refine=True, depth="sparse", match="klt")


def test_binding_checks_its_parameters():
    P = _native.Context.direct_kp_params
    assert P() == (3, 4, 5, 8, 10.0, 0.1, 64)
    assert P(levels=np.int64(2), iters=9, patch=7, grad_min=0, huber=2, z_min=0, min_pixels=6) == (2, 9, 7, 0, 2.0, 0.0, 6)
    for kw in (dict(levels=0), dict(levels=5), dict(iters=0), dict(iters=21), dict(patch=4), dict(patch=0), dict(patch=9), dict(patch=3.0),
               dict(patch=True), dict(grad_min=-1), dict(grad_min=256), dict(grad_min=8.0), dict(huber=0), dict(huber=float("nan")),
               dict(z_min=-0.1), dict(z_min=float("inf")), dict(min_pixels=5), dict(min_pixels=True)):
        with pytest.raises(ValueError):
            P(**kw)
    assert list(inspect.signature(_native.Context.direct_align_kp).parameters)[5:] == list(inspect.signature(P).parameters)


# ---- the guard ---------------------------------------------------------------------------------------------------------------------
class _Ctx:
    """stands in for _native.Context: a scripted record, the call checked against the binding's signature"""

    def __init__(self, Rt, status=0):
        self.Rt, self.status, self.calls = np.asarray(Rt, np.float64), status, []

    def direct_align_kp(self, *a, **kw):
        b = inspect.signature(_native.Context.direct_align_kp).bind(None, *a, **kw)
        b.apply_defaults()
        self.calls.append({k: v for k, v in b.arguments.items() if k != "self"})
        return dict(status=self.status, iters_done=12, Rt=self.Rt, information=np.diag([1.0, 2, 3, 4, 5, 6]))


def _pose(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T


def _odo(Rt, status=0, skipped=0, pair=(3, 4), **kw):
    o = StereoOdometer(_Cam(), patch_refine=True, **dict(SPARSE, **kw))
    o._ctx, o._patch_pair, o.skipped_frames = _Ctx(Rt, status), pair, skipped
    return o


def test_the_call_carries_the_pair_the_pose_and_the_settings():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    o = _odo(T[:3], patch_levels=2, patch_iters=5, patch_size=7)
    o._patch(T)
    (c,) = o._ctx.calls
    assert (c["slot_a"], c["slot_b"], c["levels"], c["iters"], c["patch"]) == (3, 4, 2, 5, 7)
    assert (c["grad_min"], c["huber"], c["z_min"], c["min_pixels"]) == (8, 10.0, 0.1, 64)
    assert list(c["K4"]) == [400.0, 400.0, 320.0, 240.0] and np.array_equal(c["Rt0"], T[:3])
    d = _odo(T[:3])
    d._patch(T)
    assert (d._ctx.calls[0]["levels"], d._ctx.calls[0]["iters"], d._ctx.calls[0]["patch"]) == (3, 4, 5)


def test_guard_arithmetic():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    # inside both bounds: taken, with its information matrix
    near = _pose(0.01 + 0.04, (0.02, 0.0, 0.25 + 0.09))
    o = _odo(near[:3])
    out = o._patch(T)
    assert np.array_equal(out[:3], near[:3]) and np.array_equal(out[3], [0, 0, 0, 1])
    assert o.patch_accepted and o.patch_status == 0 and np.array_equal(o.pose_information, np.diag([1.0, 2, 3, 4, 5, 6]))
    assert o.patch_record["iters_done"] == 12
    # the motion D = T_refined T^-1 is what is bounded: past the metres, past the radians, each alone
    for moved in (_pose(0.0, (0.0, 0.0, 0.11)) @ T, _pose(0.06, (0, 0, 0)) @ T):
        o = _odo(moved[:3])
        assert o._patch(T) is T and not o.patch_accepted and o.patch_status == 0 and o.pose_information is None
    for moved in (_pose(0.0, (0.0, 0.0, 0.09)) @ T, _pose(0.04, (0, 0, 0)) @ T):
        o = _odo(moved[:3])
        assert o._patch(T) is not T and o.patch_accepted
    # a refusal never leaves the matrix of an older pose behind
    o = _odo(near[:3])
    o._patch(T)
    assert o.pose_information is not None
    o._ctx.Rt = (_pose(0.0, (0.0, 0.0, 0.11)) @ T)[:3]
    assert o._patch(T) is T and o.pose_information is None
    # scaled by the frames the pair spans, like the gates
    moved = _pose(0.0, (0.0, 0.0, 0.25)) @ T
    assert _odo(moved[:3], skipped=1)._patch(T) is T
    assert _odo(moved[:3], skipped=2)._patch(T) is not T
    # a status other than 0, or a pose that is not finite: the feature pose stands
    for status in (2, -1):
        o = _odo(near[:3], status=status)
        assert o._patch(T) is T and o.patch_status == status and not o.patch_accepted
    bad = near[:3].copy()
    bad[0, 3] = np.nan
    assert _odo(bad)._patch(T) is T
    # a guard of (0, 0) takes nothing but the feature pose itself
    assert _odo(near[:3], patch_guard=(0, 0))._patch(T) is T
    # frames that are not on the device cannot be aligned
    with pytest.raises(ValueError, match="device-resident"):
        _odo(near[:3], pair=None)._patch(T)


def test_the_guard_is_the_dense_alignments_rule():
    """_direct and _patch bound the same motion by the same arithmetic: one pose, both modes, every side of both bounds"""
    T = _pose(0.01, (0.02, 0.0, 0.25))
    dense = StereoOdometer(_Cam(), direct_refine=True)
    sparse = StereoOdometer(_Cam(), patch_refine=True, **SPARSE)
    for ang, dz in ((0.0, 0.0999), (0.0, 0.1001), (0.0499, 0.0), (0.0501, 0.0), (0.03, 0.08)):
        Tr = _pose(ang, (0.0, 0.0, dz)) @ T
        for skipped in (0, 1):
            dense.skipped_frames = sparse.skipped_frames = skipped
            assert dense._guarded(T, Tr, dense.direct_guard) == sparse._guarded(T, Tr, sparse.patch_guard) == (ang <= 0.05 * (skipped + 1) and dz <= 0.1 * (skipped + 1))


def test_the_gate_sees_the_refined_pose():
    T = _pose(0.01, (0.02, 0.0, 0.25))
    far = _pose(0.0, (0.0, 0.0, 0.09)) @ T
    o = _odo(far[:3])
    o._ctx.rodrigues = lambda R: np.zeros(3)
    assert np.array_equal(o._gate(T), np.vstack([far[:3], [0, 0, 0, 1]]))
    assert o.patch_accepted and o.pose_information is not None
    gated = _odo((_pose(0.0, (0.0, 0.0, 0.09)) @ _pose(0.0, (0.0, 0.0, 0.95)))[:3])     # taken by the guard, refused by the distance gate
    gated._ctx.rodrigues = lambda R: np.zeros(3)
    assert gated._gate(_pose(0.0, (0.0, 0.0, 0.95))) is None and gated.skip_cause == "bigdist"
    assert gated.patch_accepted and gated.pose_information is None
    nan = _odo(far[:3])
    assert nan._gate(np.full((4, 4), np.nan)) is None and nan.skip_cause == "nan" and not nan._ctx.calls      # a NaN pose is never refined
    plain = StereoOdometer(_Cam(), **SPARSE)
    plain._ctx = _Ctx(far[:3])
    plain._ctx.rodrigues = lambda R: np.zeros(3)
    assert plain._gate(T) is T and not plain._ctx.calls


# ---- header, binding, library ------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_binding_agree():
    assert "vo_direct_align_kp" in _native.SYMBOLS
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, "vo_direct_align_kp")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo355.h")).read(), flags=re.S)
    decl = re.search(r"int\s+vo_direct_align_kp\s*\(([^;]*)\)\s*;", txt).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == len(_native.lib().vo_direct_align_kp.argtypes) == 13
    names = [re.sub(r"\s*/\*.*?\*/", "", a).split()[-1].lstrip("*") for a in args]
    assert names == ["ctx", "slot_a", "slot_b", "K4", "Rt0", "levels", "iters", "patch", "grad_min", "huber", "z_min", "min_pixels", "rec_out"]
    # ints and doubles where the header has them
    ci, cd, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    want = [vp if "*" in a else cd if a.startswith("double") else ci for a in args]
    assert list(_native.lib().vo_direct_align_kp.argtypes) == want
    assert "vo_direct_rec* rec_out" in args[-1]                    # the record is vo_direct_align's, unchanged
    assert ctypes.sizeof(_native.DirectRec) == 472


def test_record_dict_renames_s_and_adds_patch():
    """direct_align_kp's dict: direct_align's, `s` replaced by `keypoints`, `patch` added -- on a stand-in library"""
    class _Lib:
        def vo_direct_align_kp(self, h, a, b, K4, Rt, levels, iters, patch, grad_min, huber, z_min, min_pixels, rec):
            r = rec._obj
            r.status, r.iters_done, r.levels, r.pad = 0, levels * iters, levels, patch
            for l in range(levels):
                r.lv[l].s = 100 - l
            self.args = (a, b, levels, iters, patch, grad_min, huber, z_min, min_pixels)
            return 0

    ctx = _native.Context.__new__(_native.Context)
    ctx._lib, ctx._h = _Lib(), None
    ctx._ck = lambda rc: None
    d = ctx.direct_align_kp(2, 3, (400.0, 400.0, 320.0, 240.0), np.eye(4), levels=2, patch=7)
    assert ctx._lib.args == (2, 3, 2, 4, 7, 8, 10.0, 0.1, 64)
    assert "s" not in d and d["keypoints"].tolist() == [100, 99] and d["patch"] == 7 and d["iters_done"] == 8
    plain = set(_native.DirectRec().as_dict())
    assert set(d) == (plain - {"s"}) | {"keypoints", "patch"}
    with pytest.raises(ValueError):
        ctx.direct_align_kp(2, 3, (400.0, 400.0, 320.0, 240.0), patch=4)
