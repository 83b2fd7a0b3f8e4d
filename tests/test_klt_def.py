"""The restatement of the Lucas-Kanade tracker (tests/klt_ref.py, to which the kernels are held bit for bit) held to the DEFINITION
(tests/klt_def.py: float64, whole images, real interpolation) on every case of tests/klt_def_cases.py, without a GPU; the caps of
the cases asserted on the definition alone; and the proof that the checks can refuse: eighteen one-field mutants of the definition,
each refused on the restatement's output by at least one case.  tests/test_gpu_klt_definitions.py holds the device to the same."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_def as D                        # noqa: E402
import klt_def_cases as DC                 # noqa: E402
import klt_ref as K                        # noqa: E402

_REF = {}


def _ref(case):
    """the restatement's answer to a case's call, computed once"""
    if case["name"] not in _REF:
        got = K.track(case["a"], case["b"], case["xy"], **case["prm"])
        for v in got:
            v.setflags(write=False)
        _REF[case["name"]] = got
    return _REF[case["name"]]


def _fig(r):
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items() if not isinstance(v, np.ndarray)}


NAMES = [c["name"] for c in DC.cases()]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_held_by_the_definition(name):
    case = DC.by_name(name)
    cap = DC.caps(case)                                  # on the definition alone, first
    if case["kind"] == "pyr":
        lv = case["prm"]["levels"]
        for img in (case["a"], case["b"]):
            got = K.pyramid(img, lv)
            assert [g.shape[::-1] for g in got] == DC.level_sizes(img.shape[1], img.shape[0], lv)
            assert D.check_pyramid(got, img) == 0
    why, r = DC.hold(case, _ref(case))
    print("%s: caps %s figures %s" % (name, cap, _fig(r)))
    assert not why, why


def test_the_pattern_meets_rounding_ties():
    """(v + 128) >> 8 against floor(x + 0.5) differ from round-half-even or truncation only on exact halves: the 0 / 255 pattern
    puts at least 1 % of its output pixels there (over all shapes, and on every shape at least 4 wide and 2 high)"""
    shares = {(w, h): DC.tie_share(DC.pyr_images(w, h)[1]) for w, h in DC.PYR_SHAPES}
    print({k: round(v, 3) for k, v in shares.items()})
    assert min(v for (w, h), v in shares.items() if w >= 4 and h >= 2) >= 0.01
    assert np.mean(list(shares.values())) >= 0.01


def test_the_kernel_division_by_the_window_width():
    """k_klt_track splits a window pixel p into (p % win, p / win) as (p * ceil(65536 / win)) >> 16: exact for every odd win and every
    p a trip can produce (p < 64 x 16 = 1024)"""
    p = np.arange(1024, dtype=np.int64)
    for win in range(5, 32, 2):
        assert np.array_equal((p * ((65536 + win - 1) // win)) >> 16, p // win), win


def test_lane_sums_stay_inside_int32():
    """the largest per-lane partial sums (lane 0 of a 31 x 31 window holds 16 pixels) against 2^31, and the wave sums beyond it"""
    b, g = DC.lane_sum_bound(31)
    print("per-lane bound: b %d, G %d; 2^31 = %d" % (b, g, 2 ** 31))
    assert b == 16 * 8160 * 4080 and b < 2 ** 31 and g < 2 ** 31
    assert 31 * 31 * 4080 * 4080 > 2 ** 32               # (the whole window's sum needs the int64 wave sum)


def test_tau_is_four_times_the_measured_distance():
    """TAU_BASIS = the largest distance between track_def and the restatement over the tracked, decided points of the smooth whole-track
    cases, re-measured here (margins at 0: the measurement does not depend on TAU)"""
    worst = 0.0
    for case in DC.by_kind("track"):
        if "smooth" not in case["name"]:
            continue
        r = D.check(case["a"], case["b"], case["xy"], _ref(case), 0.0, **case["prm"])
        tr = (r["status"] == 0) & np.isfinite(case["xy"]).all(axis=1) & (_ref(case)[1] == 0)
        worst = max(worst, float(r["dist"][tr].max()))
        print("%s: largest distance %.5f px over %d tracked points" % (case["name"], r["dist"][tr].max(), tr.sum()))
    assert 0.75 * DC.TAU_BASIS <= worst <= DC.TAU_BASIS, worst
    assert DC.TAU == 4 * DC.TAU_BASIS


def test_only_the_test_build_exports_the_level_download():
    """the product library has no way to read a pyramid level back"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prod, hooks = (os.path.join(root, "openvo_amd", n) for n in ("libvo355.so", "libvo355_hooks.so"))
    assert os.path.exists(prod) and os.path.exists(hooks), "build the libraries first (__graft_entry__.build())"
    assert not hasattr(ctypes.CDLL(prod), "vo_test_klt_level") and hasattr(ctypes.CDLL(hooks), "vo_test_klt_level")


STEP_MUT = ("half", "sobel", "dy_is_dx", "step_sign", "a12_sign", "grad_from_b", "delta_x2", "zero_outside")
CANDIDATES = {m: ("step",) for m in STEP_MUT}
CANDIDATES.update({m: ("pyr",) for m in ("pyr_121", "pyr_edge", "pyr_floor", "pyr_size")})
CANDIDATES.update(eig_max=("eig",), eig_win=("eig",), lost_edge=("narrow", "track-smooth-win9-l2"), osc_full=("track-osc", "track-osc-level0"),
                  fb_unsquared=("fb", "track-smooth-win9-l2"), fb_from_forward=("fb", "track-smooth-win9-l2"))


@pytest.mark.parametrize("mut", D.MUTANTS)
def test_every_mutant_is_refused_somewhere(mut):
    """one wrong reading at a time: the restatement's output must NOT be held by the mutated definition on at least one case"""
    cs = [c for c in DC.cases() if c["kind"] in CANDIDATES[mut] or c["name"] in CANDIDATES[mut]]
    refused = []
    for case in cs:
        if case["kind"] == "pyr":
            bad = sum(D.check_pyramid(K.pyramid(img, case["prm"]["levels"]), img, mut=mut) for img in (case["a"], case["b"]))
            why = ["%d pyramid pixels differ" % bad] if bad else []
        else:
            why, _ = DC.hold(case, _ref(case), mut=mut)
        if why:
            refused.append((case["name"], why[0]))
    print("mutant %-16s refused by %d of %d cases: %s" % (mut, len(refused), len(cs), "; ".join("%s (%s)" % r for r in refused[:4])))
    assert refused, "the mutant %s is accepted on every one of its %d cases" % (mut, len(cs))
