"""Host side of the fused stereo PnP step (vo_pnp_pair): the ABI, the binding, the constructor argument and the decisions
StereoOdometer._pair_pnp_fused takes on the record the native step returns (scripted: no GPU)."""
import ctypes
import inspect

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native


def test_library_exports_the_pnp_pair_entries():
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ("vo_pnp_pair", "vo_pnp_pair_begin", "vo_pnp_pair_end"):
        assert hasattr(L, name), "libvo355.so does not export %s" % name
        assert name in _native.SYMBOLS


def test_context_has_the_pnp_pair_methods():
    for name in ("pnp_pair", "pnp_pair_begin", "pnp_pair_end"):
        assert callable(getattr(_native.Context, name, None)), name


def test_constructor_validates_pnp_refine():
    assert StereoOdometer(None, pose_method="pnp").pnp_refine == 0
    assert StereoOdometer(None, pose_method="pnp", pnp_refine=3).pnp_refine == 3
    assert StereoOdometer(None, pose_method="pnp", pnp_refine=np.int64(20)).pnp_refine == 20
    for bad in (-1, 21, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            StereoOdometer(None, pose_method="pnp", pnp_refine=bad)
    assert StereoOdometer._pnp_fused is True


class _Stereo:
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 500.0], [0, 0, 2.0, 0]])

    def slot_key(self, s):
        return (s, 0)


def _bound(fn, *a, **kw):
    """the arguments as the REAL binding (_native.Context.<fn>) would receive them, defaults applied"""
    b = inspect.signature(getattr(_native.Context, fn)).bind(None, *a, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k != "self"}


class _Ctx:
    """stands in for _native.Context: hands out the scripted record and remembers how it was asked -- every call is bound
    against the real method's signature, so a misplaced argument shows where the native step would see it"""

    def __init__(self, rec):
        self.rec, self.calls, self.begun, self.ended = rec, [], [], []

    def pnp_pair(self, *a, **kw):
        self.calls.append(_bound("pnp_pair", *a, **kw))
        return self.rec

    def pnp_pair_begin(self, *a, **kw):
        self.begun.append(_bound("pnp_pair_begin", *a, **kw))
        return 40 + len(self.begun)

    def pnp_pair_end(self, ticket):
        self.ended.append(ticket)
        return self.rec

    def pose_pair_end(self, ticket):
        raise AssertionError("a PnP ticket must be ended by pnp_pair_end")

    @staticmethod
    def rodrigues(R):
        return _native.Context.rodrigues(R)


def _rt(angle, dist):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, dist], [0, 1, 0, 0], [-s, 0, c, 0]], np.float64)


WIN, REF = _rt(0.01, 0.20), _rt(0.02, 0.25)


def _rec(M=50, n=40, best_count=30, flags=0, status=0, Rt=WIN, Rtr=REF):
    return dict(matches=M, n=n, best_iter=7, best_count=best_count, flags=flags, Rt=Rt, Rt_refined=Rtr, refine_status=status,
                refine_steps=3 if status == 0 else 0)


def _odo(rec, **kw):
    od = StereoOdometer(None, pose_method="pnp", **kw)
    od.stereo, od._ctx, od.skip_cause = _Stereo(), _Ctx(rec), "init"
    return od


@pytest.mark.parametrize("rec,cause", [
    (_rec(M=9), "matches"),                          # 1. fewer matches than min_matches
    (_rec(M=9, flags=1), "matches"),                 #    ... decided before the lookup flag is looked at
    (_rec(n=9), "matches"),                          # 3. fewer usable correspondences than max(min_matches, 4)
    (_rec(best_count=9), "outlier"),                 # 4. the winner has fewer inliers than min_matches
    (_rec(Rtr=_rt(0.02, 1.5)), "bigdist"),           # 5. the gates, on the refined pose
    (_rec(Rtr=_rt(1.2, 0.2)), "bigrot"),
    (_rec(Rtr=np.full((3, 4), np.nan)), "nan"),
])
def test_decision_table_skip_causes(rec, cause):
    od = _odo(rec, pnp_refine=3)
    assert od._pair_pnp_fused(0, 1) is None
    assert od.skip_cause == cause


def test_small_min_matches_still_needs_four_correspondences():
    od = _odo(_rec(M=3, n=3, best_count=0, status=1, Rt=np.zeros((3, 4))), min_matches=2)
    assert od._pair_pnp_fused(0, 1) is None and od.skip_cause == "matches"


def test_lookup_without_a_tap_raises_like_the_reference():
    od = _odo(_rec(flags=1))
    with pytest.raises(ZeroDivisionError):
        od._pair_pnp_fused(0, 1)


def test_refined_pose_is_used_when_the_refinement_succeeded_and_the_winner_otherwise():
    od = _odo(_rec(status=0), pnp_refine=3)
    T = od._pair_pnp_fused(0, 1)
    assert np.array_equal(T[:3], REF) and np.array_equal(T[3], [0, 0, 0, 1]) and od.skip_cause == "init"
    for status in (-1, 1):                           # failed / not attempted: the winner, gated as the winner
        od = _odo(_rec(status=status, Rtr=_rt(0.02, 5.0)), pnp_refine=3)
        T = od._pair_pnp_fused(0, 1)
        assert np.array_equal(T[:3], WIN) and od.skip_cause == "init"
    od = _odo(_rec(status=-1, Rt=_rt(0.01, 1.5)), pnp_refine=3)
    assert od._pair_pnp_fused(0, 1) is None and od.skip_cause == "bigdist"


def test_gates_widen_with_skipped_frames():
    od = _odo(_rec(Rtr=_rt(0.02, 1.5)), pnp_refine=3)
    od.skipped_frames = 1
    assert od._pair_pnp_fused(0, 1) is not None


def test_parameters_reach_the_native_step_and_tickets_are_looked_up_by_them():
    od = _odo(_rec(), pnp_refine=3, pnp_iters=128, pnp_threshold=2.0, pnp_seed=9, match_threshold=0.7, cross_check=True)
    params = od._pose_params()
    assert params == ("pnp", 0.7, (500.0, 500.0, 320.0, 240.0), 128, 2.0, 9, 3, True)
    od._pair_pnp_fused(4, 5)
    want = dict(slot_a=4, slot_b=5, ratio=0.7, K4=(500.0, 500.0, 320.0, 240.0), iters=128, thr=2.0, seed=9, refine=3,
                want_matches=False, cross_check=True)
    assert od._ctx.calls == [want]
    assert od._step_begin(4, 5, params) == 41 and od._ctx.begun == [want]     # a step begun ahead gets the same arguments
    plain = _odo(_rec())
    plain._pair_pnp_fused(1, 2)
    assert plain._ctx.calls == [dict(slot_a=1, slot_b=2, ratio=0.8, K4=(500.0, 500.0, 320.0, 240.0), iters=256, thr=1.5, seed=4321,
                                     refine=0, want_matches=False, cross_check=False)]
    # a step begun ahead with the same parameters is collected instead of computed ...
    od._specs[((4, 0), (5, 0), params)] = 2
    od._pair_pnp_fused(4, 5)
    assert od._ctx.ended == [2] and len(od._ctx.calls) == 1 and not od._specs
    # ... one begun with other parameters is not, and _drop_specs ends it with the _end of its kind
    od._specs[((4, 0), (5, 0), params[:6] + (0,) + params[7:])] = 6
    od._pair_pnp_fused(4, 5)
    assert len(od._ctx.calls) == 2 and len(od._specs) == 1
    od._drop_specs()
    assert od._ctx.ended == [2, 6] and not od._specs
    # the Umeyama mode's parameters and look-ahead condition are what they were
    um = StereoOdometer(None)
    assert um._pose_params() == (0.8, 10, 0.0, 0.0, False)


def test_fused_ok_covers_pnp_unless_forced_off():
    od = _odo(_rec())
    od.matcher = None
    assert not od._fused_ok()                        # (no plain BFMatcher)
    from openvo_amd.features import BFMatcher
    od.matcher = BFMatcher.__new__(BFMatcher)
    assert od._fused_ok()
    od._pnp_fused = False
    assert not od._fused_ok()


def test_replaced_context_calls_of_the_composed_path_keep_that_path():
    """point_clouds / ransac_pnp replaced on the context object (a spy, a substitute) are seams of the PnP mode: the fused step
    would bypass them, so it is not taken and nothing is begun ahead."""
    from openvo_amd.features import BFMatcher
    od = _odo(_rec())
    od.matcher = BFMatcher.__new__(BFMatcher)
    assert od._pnp_fused_ok() and od._fused_ok()
    for name in ("point_clouds", "ransac_pnp"):
        setattr(od._ctx, name, lambda *a, **k: None)
        assert not od._pnp_fused_ok() and not od._fused_ok()
        delattr(od._ctx, name)
    assert od._pnp_fused_ok()
