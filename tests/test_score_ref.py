"""tests/score_ref.py (the float64 definitions of the two inlier tests, with the error bound of their float32 evaluation) held to
known answers, to a numpy float32 evaluation, and to the CPU oracle on the scenes of tests/score_scenes.py -- no GPU.

    known answers      a pair with vertical disparity dy under sideways motion has d2 = dy^2 / 2; a point's reprojection error
    the bound          a float32 evaluation in numpy (one rounding per operation) never contradicts a decidable point
    (a) the oracle     oracle.ransac_essential (solvers 5 and 8) and oracle.ransac_pnp: no decidable point disagrees, at most 2 %
                       of a scene undecidable, the winner rule
    (b) power          the wrong definitions of score_ref.WRONG_*: every scene has one that moves a decidable point, the large scenes
                       are moved by every one that applies to them, and every one has its scenes
    generators         the oracle's hypotheses at n = 8 / 6 / 4 meet the bars the device is held to (so the scenes are valid)

Figures of the oracle on these scenes (printed by the tests).  Undecidable share: Sampson 0 at thr 1 and 5, at most 1.50 % at thr 0.1
on 3840 x 2160; reprojection at most 0.27 % (thr 0.1, 3840 x 2160, depths to 400 m); 44 % with the 3-D points 1e4 m from the origin.
Eight-point at n = 8: 256 of 256 hypotheses count 8 in each of 20 scenes, residual at most 1.0049 x LAPACK's.  Five-point at n = 6:
234 .. 256 hypotheses count 6.  P3P at n = 4: every hypothesis counts 4; Rt 5e-14 from the planted pose on exact data, 1.5e-6
(median) .. 2e-5 on generic points with float32-rounded pixels."""
import numpy as np
import pytest

import score_ref as SR
import score_scenes as SS

SOLVERS = (8, 5)


@pytest.fixture(scope="module")
def ess_runs(oracle):
    """(case, solver) -> (scene, thr, the oracle's result), computed once"""
    out = {}
    for case in SS.ESS_CASES:
        for solver in SOLVERS:
            s, n, iters, thr = SS.ess_case_scene(case, solver)
            out[case, solver] = (s, thr, oracle.ransac_essential(s["p1"], s["p2"], s["K4"], iters, thr, SS.SEED, solver=solver))
    return out


@pytest.fixture(scope="module")
def pnp_runs(oracle):
    out = {}
    for case in SS.PNP_CASES + [SS.PNP_OFFSET_CASE]:
        s, n, iters, thr = SS.pnp_case_scene(case)
        out[case] = (s, thr, oracle.ransac_pnp(s["X"], s["uv"], s["K4"], iters, thr, SS.SEED))
    return out


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_sampson_is_half_the_squared_vertical_disparity_under_sideways_motion():
    E = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])                  # [t]x, t = (1, 0, 0), R = I
    dy = np.array([0.0, 0.25, 1.0, 1.4, 1.5, 3.0, -2.0])
    p1 = np.stack([np.linspace(10, 600, len(dy)), np.linspace(30, 400, len(dy))], 1).astype(np.float32)
    p2 = (p1.astype(np.float64) + np.stack([np.linspace(-40, 5, len(dy)), dy], 1)).astype(np.float32)
    dy32 = p2[:, 1].astype(np.float64) - p1[:, 1]
    for K4 in (SS.K_VGA, SS.K_4K, (700.0, 700.0, 0.0, 0.0)):
        d = SR.sampson(E, K4, p1, p2, 1.0)
        assert np.allclose(d.value, dy32 ** 2 / 2, rtol=1e-9, atol=1e-12)
        assert list(d.inlier) == [bool(v * v / 2 < 1.0) for v in dy32]
        assert not SR.undecidable(d).any() and np.array_equal(d.sure_in, d.inlier)
    # the threshold is squared, and it is float32(thr): 1.4^2 / 2 = 0.98 is inside 1.0 and outside 0.98
    assert SR.sampson(E, SS.K_VGA, p1, p2, 1.0).inlier[3] and not SR.sampson(E, SS.K_VGA, p1, p2, 0.98).inlier[3]


def test_reprojection_error_and_depth_rule():
    Rt = np.c_[np.eye(3), [0.0, 0.0, 0.0]]
    X = np.array([[1.0, 2.0, 4.0], [1.0, 2.0, 4.0], [1.0, 2.0, -4.0], [1.0, 2.0, 0.0]], np.float32)
    K4 = (700.0, 650.0, 10.0, 20.0)
    uv = np.array([[700 * 0.25 + 10 + 3, 650 * 0.5 + 20 - 4], [700 * 0.25 + 10, 650 * 0.5 + 20 + 0.5], [700 * -0.25 + 10, 650 * -0.5 + 20], [10, 20]], np.float32)
    d = SR.reproj(Rt, K4, X, uv, 5.0)
    assert np.allclose(d.value[:2], [25.0, 0.25]) and np.isinf(d.value[2:]).all()
    assert list(d.inlier) == [False, True, False, False] and list(d.sure_in) == [False, True, False, False]
    assert list(d.sure_out) == [False, False, True, True]                 # 25 = 5^2 exactly: `<` keeps it out, float32 cannot promise it
    assert SR.reproj(Rt, K4, X, uv, 5.001).sure_in[0]
    assert SR.wrong_no_depth_rule(Rt, K4, X, uv, 5.0)[2] and SR.wrong_focals_swapped(Rt, K4, X, uv, 5.0)[1] == False  # noqa: E712


def test_nan_points_and_an_empty_model_are_outliers():
    s, bad = SS.nan_scene()
    E = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    d = SR.sampson(E, s["K4"], s["p1"], s["p2"], 1.0)
    assert d.sure_out[bad].all() and not d.inlier[bad].any() and not d.sure_in[bad].any()
    assert SR.sampson(np.zeros((3, 3)), s["K4"], s["p1"], s["p2"], 1.0).sure_out.all()
    p = SS.pnp_scene(20, SS.K_VGA, 1)
    assert SR.reproj(np.zeros((3, 4)), p["K4"], p["X"], p["uv"], 1.0).sure_out.all()
    p["X"][3, 1] = np.nan
    p["uv"][5, 0] = np.nan
    d = SR.reproj(p["Rt"], p["K4"], p["X"], p["uv"], 1.0)
    assert d.sure_out[[3, 5]].all() and not d.inlier[[3, 5]].any()


# ---- the bound against a float32 evaluation in numpy --------------------------------------------------------------------------
def _f32_sampson(E, K4, p1, p2, thr):
    F = SR.fundamental(E, K4)[0].astype(np.float32)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    fx0, fx1, fx2 = (F[0, 0] * u1 + F[0, 1] * v1) + F[0, 2], (F[1, 0] * u1 + F[1, 1] * v1) + F[1, 2], (F[2, 0] * u1 + F[2, 1] * v1) + F[2, 2]
    ft0, ft1 = (F[0, 0] * u2 + F[1, 0] * v2) + F[2, 0], (F[0, 1] * u2 + F[1, 1] * v2) + F[2, 1]
    num = (u2 * fx0 + v2 * fx1) + fx2
    den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1
    assert num.dtype == np.float32 and den.dtype == np.float32
    with np.errstate(all="ignore"):
        return (num * num) / den < np.float32(thr) * np.float32(thr)


def _f32_reproj(Rt, K4, X, uv, thr):
    P = SR.projection(Rt, K4)[0].astype(np.float32)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    xc, yc, zc = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))
    du, dv = xc - uv[:, 0] * zc, yc - uv[:, 1] * zc
    assert du.dtype == np.float32
    return (zc > 0) & (du * du + dv * dv < (np.float32(thr) * np.float32(thr)) * (zc * zc))


def test_a_float32_evaluation_never_contradicts_a_decidable_point(ess_runs, pnp_runs):
    """numpy float32 arithmetic: one rounding per operation, the kernel's order -- under the TRUE model and under the winners"""
    for (case, solver), (s, thr, r) in ess_runs.items():
        Et = np.array([[0, -s["t"][2], s["t"][1]], [s["t"][2], 0, -s["t"][0]], [-s["t"][1], s["t"][0], 0]]) @ s["R"]
        for E in (Et, r["E"]):
            for t in (0.1, 1.0, 5.0):
                assert len(SR.disagreements(SR.sampson(E, s["K4"], s["p1"], s["p2"], t), _f32_sampson(E, s["K4"], s["p1"], s["p2"], t))) == 0
    for case, (s, thr, r) in pnp_runs.items():
        for Rt in (s["Rt"], r["Rt"]):
            for t in (0.1, 1.0, 5.0):
                assert len(SR.disagreements(SR.reproj(Rt, s["K4"], s["X"], s["uv"], t), _f32_reproj(Rt, s["K4"], s["X"], s["uv"], t))) == 0


# ---- (a) the oracle's masks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", SS.ESS_CASES, ids=SS.case_id)
def test_oracle_sampson_mask_is_the_definition(ess_runs, case, solver):
    s, thr, r = ess_runs[case, solver]
    d = SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], thr)
    share = float(SR.undecidable(d).mean())
    print("%s solver %d: best %d @ %d, undecidable %.4f" % (SS.case_id(case), solver, r["best_count"], r["best_iter"], share))
    bad = SR.disagreements(d, r["mask"])
    assert len(bad) == 0, (bad, d.value[bad])
    assert share <= SS.CAP
    SS.winner_rule(r)


@pytest.mark.parametrize("case", SS.PNP_CASES + [SS.PNP_OFFSET_CASE], ids=SS.case_id)
def test_oracle_reprojection_mask_is_the_definition(pnp_runs, case):
    s, thr, r = pnp_runs[case]
    d = SR.reproj(r["Rt"], s["K4"], s["X"], s["uv"], thr)
    share = float(SR.undecidable(d).mean())
    print("%s: best %d @ %d, undecidable %.4f" % (SS.case_id(case), r["best_count"], r["best_iter"], share))
    bad = SR.disagreements(d, r["mask"])
    assert len(bad) == 0, (bad, d.value[bad])
    assert not r["mask"][s["behind"]].any() and d.sure_out[s["behind"]].all()
    if case is not SS.PNP_OFFSET_CASE:                # (3-D points 1e4 m from the origin: the share is a figure, not a bar)
        assert share <= SS.CAP
    SS.winner_rule(r)


# ---- (b) the power of the test ------------------------------------------------------------------------------------------------
# A scene is valid for a wrong definition when that definition moves one of its decidable points.  Every scene is valid for at
# least one (so a mask that passes there cannot come from ALL of them); the 3000-point scenes with 300 hypotheses, whose winners
# are good models, are valid for every one that applies to their camera and threshold; and every wrong definition has its scenes.
def _moved_sampson(run):
    s, thr, r = run
    d = SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], thr)
    return {name: len(SR.disagreements(d, fn(r["E"], s["K4"], s["p1"], s["p2"], thr)))
            for name, (fn, applies) in SR.WRONG_SAMPSON.items() if applies(s["K4"], thr)}


def _moved_reproj(run):
    s, thr, r = run
    d = SR.reproj(r["Rt"], s["K4"], s["X"], s["uv"], thr)
    return {name: len(SR.disagreements(d, fn(r["Rt"], s["K4"], s["X"], s["uv"], thr)))
            for name, (fn, applies) in SR.WRONG_REPROJ.items() if applies(s["K4"], thr, len(s["behind"]) > 0)}


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", SS.ESS_CASES, ids=SS.case_id)
def test_wrong_sampson_definitions_move_decidable_points(ess_runs, case, solver):
    moved = _moved_sampson(ess_runs[case, solver])
    print(SS.case_id(case), solver, moved)
    assert any(moved.values()), moved
    if case[0] >= 3000 and case[1] >= 300:
        assert all(moved.values()), moved


@pytest.mark.parametrize("case", SS.PNP_CASES, ids=SS.case_id)
def test_wrong_reprojection_definitions_move_decidable_points(pnp_runs, case):
    moved = _moved_reproj(pnp_runs[case])
    print(SS.case_id(case), moved)
    assert any(moved.values()), moved
    if case[0] >= 3000 and case[1] >= 300:
        assert all(moved.values()), moved


def test_the_planted_and_the_nan_scenes_are_valid_too(oracle):
    """the scenes the fused steps and the NaN case run on the device: every wrong definition that applies moves them"""
    nan = SS.nan_scene()[0]
    runs = [(SS.fused_essential_scene(solver), SS.FUSED_ITERS, solver) for solver in SOLVERS] + [(nan, 300, solver) for solver in SOLVERS]
    for s, iters, solver in runs:
        r = oracle.ransac_essential(s["p1"], s["p2"], s["K4"], iters, SS.FUSED_THR, SS.SEED, solver=solver)
        assert len(SR.disagreements(SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], SS.FUSED_THR), r["mask"])) == 0
        moved = _moved_sampson((s, SS.FUSED_THR, r))
        assert moved and all(moved.values()), moved
    s = SS.fused_pnp_scene()
    r = oracle.ransac_pnp(s["X"], s["uv"], s["K4"], SS.FUSED_ITERS, SS.FUSED_THR, SS.SEED)
    moved = _moved_reproj((s, SS.FUSED_THR, r))
    assert moved and all(moved.values()), moved


@pytest.mark.parametrize("K4", [SS.GEN_K4, SS.K_VGA], ids=["hd", "vga"])
@pytest.mark.parametrize("iters", SS.TIE_ITERS)
def test_the_tie_scenes_give_ties(oracle, iters, K4):
    """the scenes of the device's tie cases: several hypotheses hold the largest count, and the oracle picks the first of them"""
    for solver in SOLVERS:
        s = SS.tie_scene(solver, K4)
        r = oracle.ransac_essential(s["p1"], s["p2"], s["K4"], iters, SS.GEN_THR, SS.SEED, solver=solver)
        assert len(SR.disagreements(SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], SS.GEN_THR), r["mask"])) == 0
        SS.tie_rule(r)
        print("solver %d, %d hypotheses: %d hold the largest count %d" % (solver, iters, SS.ties(r["counts"]), r["best_count"]))
    s = SS.tie_scene("pnp", K4)
    r = oracle.ransac_pnp(s["X"], s["p2"], s["K4"], iters, SS.GEN_THR, SS.SEED)
    assert len(SR.disagreements(SR.reproj(r["Rt"], s["K4"], s["X"], s["p2"], SS.GEN_THR), r["mask"])) == 0
    SS.tie_rule(r)
    print("PnP, %d hypotheses: %d hold the largest count %d" % (iters, SS.ties(r["counts"]), r["best_count"]))


def test_every_wrong_definition_has_a_valid_scene(ess_runs, pnp_runs):
    for name in SR.WRONG_SAMPSON:
        for solver in SOLVERS:
            assert any(_moved_sampson(ess_runs[c, solver]).get(name, 0) for c in SS.ESS_CASES), (name, solver)
    for name in SR.WRONG_REPROJ:
        assert any(_moved_reproj(pnp_runs[c]).get(name, 0) for c in SS.PNP_CASES), name


# ---- the generators, on the oracle ---------------------------------------------------------------------------------------------
def test_oracle_eight_point_hypotheses_are_exact_at_n8(oracle):
    worst_full, worst_ratio = SS.GEN_ITERS, 0.0
    for seed in range(SS.GEN_SEEDS):
        s = SS.exact_scene(8, seed)
        full, ratio = SS.check_eight_point(oracle.ransac_essential(s["p1"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed), s)
        worst_full, worst_ratio = min(worst_full, full), max(worst_ratio, ratio)
    print("eight-point: at least %d of %d hypotheses count 8, residual ratio to LAPACK at most %.4f" % (worst_full, SS.GEN_ITERS, worst_ratio))


def test_oracle_five_point_winner_is_an_essential_matrix_at_n6(oracle):
    figs = []
    for seed in range(SS.GEN_SEEDS):
        s = SS.exact_scene(6, seed)
        figs.append(SS.check_five_point(oracle.ransac_essential(s["p1"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed, solver=5), s))
    SS.check_five_point_over_scenes([f[0] for f in figs], [f[1] for f in figs])
    print("five-point: hypotheses that count 6 per scene:", [f[2] for f in figs])


def test_oracle_p3p_hypotheses_are_exact_at_n4(oracle):
    worst, generic = 0.0, []
    for seed in range(SS.GEN_SEEDS):
        s = SS.dyadic_pnp_scene(seed)
        worst = max(worst, SS.check_p3p(oracle.ransac_pnp(s["X"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed), s))
        s = SS.exact_scene(4, seed)                   # generic points, float32-rounded pixels: every count, the pose as a figure
        generic.append(SS.check_p3p(oracle.ransac_pnp(s["X"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed), s, bar=None))
    print("P3P: Rt within %.3g of the planted pose on exact data; generic scenes: median %.3g, largest %.3g" % (worst, np.median(generic), max(generic)))
