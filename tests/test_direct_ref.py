"""The restatement of the dense direct alignment (tests/direct_ref.py) on the planted cases (tests/direct_cases.py) and on the
synthetic corridor, without a GPU: what the device test (tests/test_gpu_direct.py) compares the kernel with has to be worth it.

    regimes        every case ends with the status its name promises, within its bounds on the completed iterations, with the lattice
                   step, the Huber weights and the smaller selection it was built for -- and with a decision margin >= 1e-6, which is
                   what lets the device's integer fields be compared exactly
    improvement    the planted cases start 2 - 3 px of level-0 flow off the planted pose (the identity against PLANTED) and end
                   closer to it; asserted: at least HALF the factor measured here (translation error before / after)
    corridor       C1 (640 x 480), frames 0 - 7, the oracle's SGBM + median3x3_s16, every pair from the identity: the end-point
                   error table the README quotes is recomputed and printed; asserted: the 16384-point chain ends nearer to the ground
                   truth than 0.044 m, the README's sparse-PnP figure for the same stretch

Measured here (translation error in metres before -> after, factor; rotation error after in radians):
    levels1      0.05766 -> 0.00031  184   1.6e-04        step2        0.05766 -> 0.00101   57   5.0e-04
    levels2      0.05766 -> 0.00020  283   6.0e-05        step5        0.05766 -> 0.00091   63   4.2e-04
    levels3      0.05766 -> 0.00084   69   3.9e-04        roi          0.05766 -> 0.00164   35   8.6e-04
    levels4      0.05766 -> 0.00029  196   1.3e-04        huber        0.05766 -> 0.01934  3.0   8.4e-03
    odd_levels3  0.05766 -> 0.00079   73   3.8e-04        disp_range   0.05766 -> 0.00192   30   8.7e-04
    odd_levels4  0.05766 -> 0.00100   58   4.6e-04        small        0.05766 -> 0.00069   83   4.6e-04
(the remaining error is the disparity's 1 / 16 px quantisation and the images' rounding to uint8; the occluder of `huber` covers 4 % of
B and its edge pulls the fit: Huber weights bound an outlier's pull, they do not remove it)
Corridor C1, frames 0 - 7, end-point error / worst single pair:
    3 levels x 8 iterations, 16384 points   0.0039 m / 0.0011 m
    3 levels x 8 iterations,  4096 points   0.0039 m / 0.0025 m
    3 levels x 5 iterations, 16384 points   0.0719 m / 0.0431 m"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_cases as DC                  # noqa: E402
import direct_ref as DR                    # noqa: E402

# translation-error factor before / after measured with this file (the table above), to two digits; half of it is asserted
MEASURED = dict(levels1=184, levels2=283, levels3=69, levels4=196, odd_levels3=73, odd_levels4=58, small=83, step2=57, step5=63, roi=35,
                huber=3.0, disp_range=30)

_results = {}


def result(case):
    """the restatement's record of a case, computed once and shared (read-only) by the tests of this module"""
    if case.name not in _results:
        A, B, disp, Q, K4, Rt0, _ = case.build()
        _results[case.name] = DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **case.kw)
    return _results[case.name]


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_case_reaches_its_regime_with_a_decision_margin(case):
    r, e = result(case), case.expect
    total = case.kw["levels"] * case.kw["iters"]
    print("%s: status %d, %d of %d iterations, s %s, selected %s, first %s, last %s, margin %.2e, Huber-weighted terms %d"
          % (case.name, r["status"], r["iters_done"], total, r["s"].tolist(), r["selected"].tolist(), r["n_first"].tolist(), r["n_last"].tolist(),
             r["margin"], r["n_huber"]))
    assert r["margin"] >= DC.MARGIN
    assert r["status"] == e["status"]
    if e["status"] == 0:
        assert r["iters_done"] == total and (r["n_last"] >= case.kw["min_pixels"]).all()
    else:
        assert e["done"][0] <= r["iters_done"] <= e["done"][1] and r["iters_done"] < total
    if "s0" in e:
        assert r["s"][0] == e["s0"]
    if e.get("huber"):
        assert r["n_huber"] > 0
        A, B, disp, Q, K4, Rt0, _ = case.build()
        assert DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **dict(case.kw, huber=1e6))["n_huber"] == 0
    if e.get("fewer"):                                  # the disparity range removes points the full range keeps
        A, B, disp, Q, K4, Rt0, _ = case.build()
        full = DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **dict(case.kw, dmin=4.0, dmax=100.0))
        assert (r["selected"] < full["selected"]).all() and (r["selected"] > 0).all()
    if case.roi is not None:
        A, B, disp, Q, K4, Rt0, _ = case.build()
        assert (r["selected"] < DR.align(A, B, disp, Q, K4, Rt0, **case.kw)["selected"]).all()
    if case.name == "bad_pivot":                        # the layout, not an accident: no vertical gradient, so H[4][4] is exactly 0
        assert r["trace"][0]["n"] >= case.kw["min_pixels"] and len(r["trace"]) == 1
    if case.name == "starved_midway":
        assert r["trace"][0]["n"] >= case.kw["min_pixels"] > r["trace"][-1]["n"]
    if case.name == "constant":
        assert not r["selected"].any()


def test_every_regime_of_the_matrix_is_present():
    kws = [c.kw for c in DC.CASES]
    assert {k["levels"] for k in kws} == {1, 2, 3, 4}
    assert {(c.w, c.h) for c in DC.CASES} == {(96, 72), (97, 61), (64, 48)}
    assert {c.expect["status"] for c in DC.CASES} == {0, 2, -1}
    assert any(c.roi for c in DC.CASES) and {c.expect.get("s0") for c in DC.CASES} >= {2, 5}


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.planted], ids=lambda c: c.name)
def test_planted_cases_end_closer_to_the_planted_pose(case):
    r = result(case)
    _, _, _, _, _, Rt0, truth = case.build()
    (t0, a0), (t1, a1) = DC.pose_error(Rt0, truth), DC.pose_error(r["Rt"], truth)
    print("%-12s %.5f -> %.5f m (factor %.3g; asserted %.3g), %.1e -> %.1e rad" % (case.name, t0, t1, t0 / t1, MEASURED[case.name] / 2, a0, a1))
    assert 0.05 < t0 < 0.07                            # 2 - 3 px of flow at f = 0.9 w and 1.9 m
    assert t1 < t0 and a1 < a0
    assert t0 / t1 >= MEASURED[case.name] / 2


def test_corridor_chain_from_the_identity():
    from oracle import oracle as O
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    pairs = c.pairs(0, 8)
    disp = [O.median3x3_s16(O.sgbm_compute(L, R, c.sgbm_params())) for L, R in pairs[:7]]
    K4 = (c.f, c.f, c.cx, c.cy)
    ends = {}
    for name, kw in (("3 x 8, 16384 points", {}), ("3 x 8, 4096 points", dict(max_points=4096)), ("3 x 5, 16384 points", dict(iters=5))):
        T, worst = np.eye(4), 0.0
        for k in range(7):
            r = DR.align(pairs[k][0], pairs[k + 1][0], disp[k], c.Q(), K4, **kw)
            assert r["status"] == 0
            Tk = np.vstack([r["Rt"], [0, 0, 0, 1]])
            gt = np.linalg.inv(c.gt_pose(k + 1)) @ c.gt_pose(k)
            worst = max(worst, float(np.linalg.norm((Tk @ np.linalg.inv(gt))[:3, 3])))
            T = Tk @ T
        ends[name] = float(np.linalg.norm(np.linalg.inv(T)[:3, 3] - c.gt_pose(7)[:3, 3]))
        print("%-22s end-point error %.4f m, worst single pair %.4f m" % (name, ends[name], worst))
    assert ends["3 x 8, 16384 points"] < 0.044
