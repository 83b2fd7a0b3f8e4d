"""The RANSAC fronts of csrc/ransac.hip and csrc/fivept.inc held to what their results MEAN, not to their restatement:

    masks        k_ransac_score / k_ransac_mask (ransac_essential, solvers 8 and 5), k_pnp_score / k_pnp_mask (ransac_pnp), and the
                 fused finishes k_mono_finish (mono_pair_begin / _end), k_mono_pose_finish (mono_pose_pair) and k_pnp_finish (pnp_pair,
                 map_track): the mask against tests/score_ref.py -- the float64 definition of the Sampson and the reprojection test,
                 evaluated with the model the device returned.  Every point the float32 error bound can decide must agree, at most
                 2 % of a scene may be undecidable, best_count == mask.sum() == counts[best_iter], and best_iter is the lowest index
                 of the largest count.  tests/test_score_ref.py shows on the CPU that a two-term denominator, an unsquared
                 threshold, a transposed E, a missing depth rule or swapped focal lengths each move decidable points of these scenes.
    generators   k_ransac_hyp at n = 8, k_ransac_hyp5 / k_ransac_roots5 at n = 6, k_pnp_hyp at n = 4, where every hypothesis sees
                 every point: noise-free float32 pixels, 256 hypotheses, 20 scenes; the eight-point winner against a LAPACK solution
                 of the same system, the five-point winner against the constraints that define an essential matrix, P3P against
                 the planted pose (to 1e-6 where points and pixels are exact in float32: score_scenes.dyadic_pnp_scene says why;
                 on generic points every count is asserted and the distance printed).
    NaN          three of 65 correspondences NaN in both views: outliers, and the other 62 as the definition has them.
    ties         n = 8 / 6 / 4 noise-free points and 257 or 1025 hypotheses: many hold the full count, so the winner is the tie-break's
                 (the lowest index, np.argmax's), and the block-wide argmax of every entry takes a second trip through the counts.
                 The fused steps return no counts: theirs are the stand-alone entry's on the same correspondences.

The cases are tests/score_scenes.py.  The fused steps run on planted slots in one child process against the test-only library.
Every test prints its figures (undecidable share, hypotheses with a full count, residual ratio)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as SR                     # noqa: E402
import score_scenes as SS                  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = (8, 5)


def _hold_mask(d, mask, what, cap=SS.CAP):
    """a mask against a Decision -> the undecidable share"""
    bad = SR.disagreements(d, mask)
    assert len(bad) == 0, "%s: %d decidable points disagree with the definition, e.g. point %d with value %.6g" % (what, len(bad), bad[0], d.value[bad[0]])
    share = float(SR.undecidable(d).mean())
    print("%s: %d inliers of %d, undecidable share %.4f" % (what, int(np.asarray(mask).sum()), len(mask), share))
    assert cap is None or share <= cap, "%s: undecidable share %.4f" % (what, share)
    return share


# ---- masks of the stand-alone entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("case", SS.ESS_CASES, ids=SS.case_id)
def test_essential_mask_is_the_sampson_definition(ctx_small, case, solver):
    s, n, iters, thr = SS.ess_case_scene(case, solver)
    r = ctx_small.ransac_essential(s["p1"], s["p2"], s["K4"], iters, thr, SS.SEED, want_counts=True, solver=solver)
    assert len(r["mask"]) == n and len(r["counts"]) == iters
    _hold_mask(SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], thr), r["mask"], "%s solver %d" % (SS.case_id(case), solver))
    SS.winner_rule(r)


@pytest.mark.parametrize("case", SS.PNP_CASES + [SS.PNP_OFFSET_CASE], ids=SS.case_id)
def test_pnp_mask_is_the_reprojection_definition(ctx_small, case):
    s, n, iters, thr = SS.pnp_case_scene(case)
    r = ctx_small.ransac_pnp(s["X"], s["uv"], s["K4"], iters, thr, SS.SEED, want_counts=True)
    assert len(r["mask"]) == n and len(r["counts"]) == iters
    d = SR.reproj(r["Rt"], s["K4"], s["X"], s["uv"], thr)
    # (3-D points 1e4 m from the origin: the share is a figure -- DESIGN.md records it -- not a bar)
    _hold_mask(d, r["mask"], SS.case_id(case), cap=None if case is SS.PNP_OFFSET_CASE else SS.CAP)
    assert not r["mask"][s["behind"]].any(), "a point behind the camera or on its plane is an inlier"
    SS.winner_rule(r)


@pytest.mark.parametrize("solver", SOLVERS)
def test_nan_correspondences_are_outliers_and_leave_the_rest_alone(ctx_small, solver):
    s, bad = SS.nan_scene()
    r = ctx_small.ransac_essential(s["p1"], s["p2"], s["K4"], 300, 1.0, SS.SEED, want_counts=True, solver=solver)
    assert not r["mask"][bad].any(), "a NaN correspondence is an inlier"
    assert np.isfinite(r["E"]).all() and r["best_count"] >= 20, (r["best_count"], r["E"])
    d = SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], 1.0)
    assert d.sure_out[bad].all()
    _hold_mask(d, r["mask"], "NaN scene, solver %d" % solver, cap=None)
    rest = np.setdiff1d(np.arange(65), bad)
    assert float(SR.undecidable(d)[rest].mean()) <= SS.CAP
    SS.winner_rule(r)


# ---- ties: the winner is the lowest index of the largest count ----------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("iters", SS.TIE_ITERS)
def test_essential_winner_among_ties_is_the_lowest_index(ctx_small, iters, solver):
    s = SS.tie_scene(solver)
    r = ctx_small.ransac_essential(s["p1"], s["p2"], s["K4"], iters, SS.GEN_THR, SS.SEED, want_counts=True, solver=solver)
    assert len(r["mask"]) == SS.TIE_N[solver] and len(r["counts"]) == iters
    _hold_mask(SR.sampson(r["E"], s["K4"], s["p1"], s["p2"], SS.GEN_THR), r["mask"], "ties, solver %d, %d hypotheses" % (solver, iters))
    SS.tie_rule(r)
    assert r["best_iter"] == int(np.argmax(r["counts"]))
    print("%d hypotheses hold the largest count %d, the winner is %d" % (SS.ties(r["counts"]), r["best_count"], r["best_iter"]))


@pytest.mark.parametrize("iters", SS.TIE_ITERS)
def test_pnp_winner_among_ties_is_the_lowest_index(ctx_small, iters):
    s = SS.tie_scene("pnp")
    r = ctx_small.ransac_pnp(s["X"], s["p2"], s["K4"], iters, SS.GEN_THR, SS.SEED, want_counts=True)
    assert len(r["mask"]) == SS.TIE_N["pnp"] and len(r["counts"]) == iters
    _hold_mask(SR.reproj(r["Rt"], s["K4"], s["X"], s["p2"], SS.GEN_THR), r["mask"], "ties, PnP, %d hypotheses" % iters)
    SS.tie_rule(r)
    assert r["best_iter"] == int(np.argmax(r["counts"]))
    print("%d hypotheses hold the largest count %d, the winner is %d" % (SS.ties(r["counts"]), r["best_count"], r["best_iter"]))


# ---- the hypothesis generators ------------------------------------------------------------------------------------------------
def test_eight_point_hypotheses_are_exact_at_n8(ctx_small):
    worst_full, worst_ratio = SS.GEN_ITERS, 0.0
    for seed in range(SS.GEN_SEEDS):
        s = SS.exact_scene(8, seed)
        r = ctx_small.ransac_essential(s["p1"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed, want_counts=True)
        full, ratio = SS.check_eight_point(r, s)
        worst_full, worst_ratio = min(worst_full, full), max(worst_ratio, ratio)
    print("eight-point: at least %d of %d hypotheses count 8, residual ratio to LAPACK at most %.4f" % (worst_full, SS.GEN_ITERS, worst_ratio))


def test_five_point_winner_is_an_essential_matrix_at_n6(ctx_small, oracle):
    figs, shares = [], []
    for seed in range(SS.GEN_SEEDS):
        s = SS.exact_scene(6, seed)
        a = (s["p1"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed)
        r = ctx_small.ransac_essential(*a, want_counts=True, solver=5)
        figs.append(SS.check_five_point(r, s))
        want = int((oracle.ransac_essential(*a, solver=5)["counts"] == 6).sum())
        assert figs[-1][2] >= want, "scene %d: %d hypotheses count 6, the oracle has %d" % (seed, figs[-1][2], want)
        shares.append(figs[-1][2] / SS.GEN_ITERS)
    SS.check_five_point_over_scenes([f[0] for f in figs], [f[1] for f in figs])
    print("five-point: share of hypotheses that count 6: least %.4f, median %.4f; |det E| at most %.3g, cubic constraint at most %.3g" % (
        min(shares), float(np.median(shares)), max(f[0] for f in figs), max(f[1] for f in figs)))


def test_p3p_hypotheses_are_exact_at_n4(ctx_small):
    worst, generic = 0.0, []
    for seed in range(SS.GEN_SEEDS):
        s = SS.dyadic_pnp_scene(seed)
        worst = max(worst, SS.check_p3p(ctx_small.ransac_pnp(s["X"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed, want_counts=True), s))
        s = SS.exact_scene(4, seed)                   # generic points, float32-rounded pixels: every count, the pose as a figure
        generic.append(SS.check_p3p(ctx_small.ransac_pnp(s["X"], s["p2"], s["K4"], SS.GEN_ITERS, SS.GEN_THR, SS.SEED + seed, want_counts=True), s, bar=None))
    print("P3P: Rt within %.3g of the planted pose on exact data; generic scenes: median %.3g, largest %.3g" % (worst, np.median(generic), max(generic)))


# ---- masks of the fused steps: in the child process -----------------------------------------------------------------------------
FUSED_NQ, FUSED_M, FUSED_ITERS, FUSED_THR, FUSED_RATIO = SS.FUSED_NQ, SS.FUSED_M, SS.FUSED_ITERS, SS.FUSED_THR, SS.FUSED_RATIO
FUSED_STEPS = ["mono_pair_8", "mono_pair_5", "mono_pair_async_8", "mono_pair_async_5", "mono_pose_pair_8", "mono_pose_pair_5", "pnp_pair", "map_track"]
# the tie scenes through the fused entries: "<step>@<hypotheses>"
TIE_STEPS = ["%s@%d" % (step, iters) for iters in SS.TIE_ITERS for step in ("mono_pair_async_8", "mono_pair_async_5", "mono_pose_pair_8",
                                                                            "mono_pose_pair_5", "pnp_pair")]
TIE_PAD = 7                                # keypoints of slot a beside the matched ones


def _plant_matches(ctx, rng, pa, pb, xyz_a=None, sa=0, sb=1, nq=FUSED_NQ):
    """two slots whose matches are the len(pa) planted pairs (FUSED_M of FUSED_NQ keypoints unless the caller has fewer): slot a's
    keypoint q[k] at pa[k] (3-D point xyz_a[k]), slot b's t[k] at pb[k]"""
    import planted as P
    dq, dt, q, t = P.descriptors(nq, len(pa), rng)
    mq, mt = P.matches(dq, dt, FUSED_RATIO)
    assert np.array_equal(mq, q) and np.array_equal(mt, t)
    xy_a = rng.uniform(0, 600, (nq, 2)).astype(np.float32)
    xy_b = rng.uniform(0, 600, (len(dt), 2)).astype(np.float32)
    Xa = P._cloud(nq, rng).astype(np.float32)
    xy_a[q], xy_b[t] = pa, pb
    if xyz_a is not None:
        Xa[q] = xyz_a
    ctx.plant_keypoints(sa, xy_a, dq, Xa)
    ctx.plant_keypoints(sb, xy_b, dt, P._cloud(len(dt), rng).astype(np.float32))
    return q, t, xy_a, xy_b, Xa


def _mono_case(ctx, name, tie_iters=0):
    """tie_iters: the tie scene of the solver under that many hypotheses in place of the planted scene"""
    import mono_pose_ref as MR
    solver = int(name.rsplit("_", 1)[1])
    s = SS.tie_scene(solver, SS.K_VGA) if tie_iters else SS.fused_essential_scene(solver)
    m, iters, thr = (len(s["p1"]), tie_iters, SS.GEN_THR) if tie_iters else (FUSED_M, FUSED_ITERS, FUSED_THR)
    q, t, xy_a, xy_b, _ = _plant_matches(ctx, np.random.default_rng([13, solver]), s["p1"], s["p2"], nq=m + TIE_PAD if tie_iters else FUSED_NQ)
    a = (0, 1, FUSED_RATIO, s["K4"])
    kw = dict(iters=iters, thr=thr, seed=SS.SEED, solver=solver)
    sync = ctx.mono_pair(*a, want_matches=True, **kw)
    if tie_iters:                                  # the counts of these correspondences: the stand-alone entry draws the same hypotheses
        ref = ctx.ransac_essential(xy_a[q], xy_b[t], s["K4"], tie_iters, thr, SS.SEED, want_counts=True, solver=solver)
        SS.tie_rule(ref)
        assert sync["best_iter"] == ref["best_iter"] == int(np.argmax(ref["counts"])) and sync["best_count"] == ref["best_count"]
        print("%s: %d of %d hypotheses hold the largest count %d, the winner is %d" % (name, SS.ties(ref["counts"]), tie_iters, ref["best_count"], ref["best_iter"]))
    if name.startswith("mono_pair_async"):
        r = ctx.mono_pair_end(ctx.mono_pair_begin(*a, want_matches=True, **kw), want_matches=True)
        assert np.array_equal(r["E"], sync["E"]) and np.array_equal(r["mask"], sync["mask"]) and r["best_iter"] == sync["best_iter"]
    else:
        r = sync
    assert r["matches"] == m and np.array_equal(r["q"], q) and np.array_equal(r["t"], t)
    d = SR.sampson(r["E"], s["K4"], xy_a[r["q"]], xy_b[r["t"]], thr)
    if not name.startswith("mono_pose"):
        share = _hold_mask(d, r["mask"], name)
        assert r["best_count"] == int(r["mask"].sum()) and r["best_count"] >= m // 2
        return dict(share=share, best_count=r["best_count"])
    # the pose step hands out no mask: its winner, its count, and the depths it leaves on the inliers' keypoints in slot b
    p = ctx.mono_pose_pair(*a, **kw)
    assert p["matches"] == m and p["best_iter"] == r["best_iter"] and np.array_equal(p["E"], r["E"]) and p["flags"] & 3 == 0
    lo, hi = int(d.sure_in.sum()), m - int(d.sure_out.sum())
    assert lo <= p["best_count"] <= hi and p["best_count"] == r["best_count"], "best_count %d, the definition allows %d .. %d" % (p["best_count"], lo, hi)
    depth, serial = ctx.download_mono_depth(1)
    assert serial == p["serial"] != 0
    has = depth[r["t"]] != 0
    assert not (has & d.sure_out).any(), "%d keypoints of sure outliers carry a depth" % int((has & d.sure_out).sum())
    z1, z2, _ = MR.depths(p["R"], p["t"], MR.normalise(xy_a[r["q"]], s["K4"]), MR.normalise(xy_b[r["t"]], s["K4"]))
    front = (z1 > 1e-6) & (z2 > 1e-6)
    missing = d.sure_in & front & ~has
    assert not missing.any(), "%d sure inliers in front of both cameras carry no depth" % int(missing.sum())
    assert int(has.sum()) == p["n_depth"] <= p["best_count"] and p["n_depth"] >= m // 2
    share = float(SR.undecidable(d).mean())
    print("%s: best_count %d in %d .. %d, %d depths, undecidable share %.4f" % (name, p["best_count"], lo, hi, p["n_depth"], share))
    assert share <= SS.CAP
    return dict(share=share, best_count=p["best_count"])


def _pnp_case(ctx, org):
    s = SS.fused_pnp_scene()
    o32 = np.float32(org)
    q, t, xy_a, xy_b, Xa = _plant_matches(ctx, np.random.default_rng(14), np.zeros((FUSED_M, 2), np.float32), s["uv"] - o32, xyz_a=s["X"])
    r = ctx.pnp_pair(0, 1, FUSED_RATIO, s["K4"], iters=FUSED_ITERS, thr=FUSED_THR, seed=SS.SEED, refine=3, want_matches=True)
    assert (r["matches"], r["n"]) == (FUSED_M, FUSED_M) and np.array_equal(r["q"], q) and np.array_equal(r["t"], t)
    X, uv = Xa[r["q"]], (xy_b[r["t"]] + o32).astype(np.float32)
    # the mask belongs to the RANSAC winner Rt (k_pnp_finish scores with P_all[best]), not to the refit
    share = _hold_mask(SR.reproj(r["Rt"], s["K4"], X, uv, FUSED_THR), r["mask"], "pnp_pair")
    assert r["best_count"] == int(r["mask"].sum()) >= FUSED_M // 2 and r["refine_status"] == 0 and not np.array_equal(r["Rt"], r["Rt_refined"])
    assert not r["mask"][s["behind"]].any(), "a point behind the camera or on its plane is an inlier"
    moved = len(SR.disagreements(SR.reproj(r["Rt_refined"], s["K4"], X, uv, FUSED_THR), r["mask"]))
    print("pnp_pair: under Rt_refined %d decidable points would disagree" % moved)
    return dict(share=share, best_count=r["best_count"])


def _pnp_tie_case(ctx, org, iters):
    s = SS.tie_scene("pnp", SS.K_VGA)
    m, o32 = len(s["X"]), np.float32(org)
    q, t, xy_a, xy_b, Xa = _plant_matches(ctx, np.random.default_rng(16), np.zeros((m, 2), np.float32), s["p2"] - o32, xyz_a=s["X"], nq=m + TIE_PAD)
    r = ctx.pnp_pair(0, 1, FUSED_RATIO, s["K4"], iters=iters, thr=SS.GEN_THR, seed=SS.SEED, refine=3, want_matches=True)
    assert (r["matches"], r["n"]) == (m, m) and np.array_equal(r["q"], q) and np.array_equal(r["t"], t)
    X, uv = Xa[r["q"]], (xy_b[r["t"]] + o32).astype(np.float32)
    ref = ctx.ransac_pnp(X, uv, s["K4"], iters, SS.GEN_THR, SS.SEED, want_counts=True)
    SS.tie_rule(ref)
    assert r["best_iter"] == ref["best_iter"] == int(np.argmax(ref["counts"])) and r["best_count"] == ref["best_count"]
    assert np.array_equal(r["Rt"], ref["Rt"]) and np.array_equal(r["mask"], ref["mask"])
    share = _hold_mask(SR.reproj(r["Rt"], s["K4"], X, uv, SS.GEN_THR), r["mask"], "pnp_pair@%d" % iters)
    assert r["best_count"] == int(r["mask"].sum()) >= m // 2
    print("pnp_pair@%d: %d hypotheses hold the largest count %d, the winner is %d" % (iters, SS.ties(ref["counts"]), ref["best_count"], ref["best_iter"]))
    return dict(share=share, best_count=r["best_count"])


def _map_case(ctx):
    import map_ref as M
    import test_gpu_map as G
    import test_gpu_map_fused as GF
    rng = np.random.default_rng(15)
    n = 330
    scene = GF.map_scene(n, rng, GF.pad_invisible(n, rng))
    pose = G.pose_cw()
    probe = M.MapRef(n, G.KP_CAP)
    GF._plant(ctx, (), probe, scene)
    f = GF.new_frame(probe.view(pose, G.K4, G.Z_MIN, G.ORG, G.CROP), rng, FUSED_M)
    h = ctx.map_create(n + 300)
    try:
        GF._plant(ctx, (h,), None, scene)
        ctx.plant_keypoints(GF.NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        r = ctx.map_track(h, GF.NEW_SLOT, GF.VIEW_SLOT, pose, G.K4, G.Z_MIN, FUSED_RATIO, FUSED_ITERS, FUSED_THR, SS.SEED, 3, 10, GF.MAXD, GF.MAXR,
                          GF.SERIAL, GF.MAX_AGE, GF.MAX_OBS)
        assert r["decision"] == 0 and r["n"] == r["matches"] >= FUSED_M // 2 and r["n"] % 64 != 0, (r["decision"], r["n"], r["matches"])
        view = ctx.peek_view(h, GF.VIEW_SLOT, n)
        X, uv = view["xyz"][r["q"]], (f["xy"][r["t"]] + np.float32(G.ORG)).astype(np.float32)
        share = _hold_mask(SR.reproj(r["Rt"], G.K4, X, uv, FUSED_THR), r["mask"], "map_track")
        assert r["best_count"] == int(r["mask"].sum()) >= r["n"] // 3
        return dict(share=share, best_count=r["best_count"])
    finally:
        ctx.map_destroy(h)


def _fused_body():
    import test_gpu_map as G
    ctx = G._context()
    out = {}
    for name in FUSED_STEPS:
        fn = (lambda: _pnp_case(ctx, G.ORG)) if name == "pnp_pair" else (lambda: _map_case(ctx)) if name == "map_track" else (lambda: _mono_case(ctx, name))
        G._guard(out, name, fn)
    for name in TIE_STEPS:
        step, iters = name.split("@")
        G._guard(out, name, (lambda: _pnp_tie_case(ctx, G.ORG, int(iters))) if step == "pnp_pair" else (lambda: _mono_case(ctx, step, int(iters))))
    ctx.close()
    print("FUSED-RESULT " + json.dumps(out))


_RESULT = []


def _child():
    if not _RESULT:
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        _RESULT.append(None)                           # (a child that ended abnormally is not started again)
        r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_ransac_definitions as t; t._fused_body()"], cwd=ROOT,
                           env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("FUSED-RESULT ")]
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("FUSED-RESULT ")))
        assert r.returncode == 0 and lines, r.stdout[-6000:] + r.stderr[-4000:]
        _RESULT[0] = json.loads(lines[-1][len("FUSED-RESULT "):])
    assert _RESULT[0] is not None, "the child process of the fused steps ended abnormally before"
    return _RESULT[0]


@pytest.mark.parametrize("name", FUSED_STEPS + TIE_STEPS)
def test_fused_step_mask_is_the_definition(name):
    res = _child()[name]
    assert res["ok"], res["err"]
    print("%s: best_count %d, undecidable share %.4f" % (name, res["best_count"], res["share"]))
