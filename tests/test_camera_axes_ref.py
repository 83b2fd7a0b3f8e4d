"""The cases of tests/test_gpu_camera_axes.py on the CPU: each is built with its generic camera (tests/camera_cases.py), run through
the reference the device is held to, and asserted

    (a) to reach the regime its name promises, with the decision margin the suite it borrows from demands, and
    (b) to be SENSITIVE to every camera a slip would produce (camera_cases.mutants: fx / fy swapped, cx / cy swapped, fy read as fx,
        the principal point taken for the image centre; for the alignment also Q[3][3] = 0 and the principal point taken from Q; for
        the reprojection every entry of Q read as zero, and Q transposed): under each mutant the reference's output differs from the
        generic camera's in a field the device test compares -- another value of an exact field, or at least 1000 x the bar of a
        field held to a bar.  That is what proves, without touching a kernel, that the device test fails on the slip.

Every figure is printed (pytest -s).  Per entry point: the smallest distance over the mutants and the field it is in."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as CC                  # noqa: E402
import direct_cases as DC                  # noqa: E402
import direct_ref as DR                    # noqa: E402
import klt_cases as C                      # noqa: E402
import klt_ref as K                        # noqa: E402
import mono_pose_ref as ref                # noqa: E402
import planted_mono as PM                  # noqa: E402
import planted_pnp as PP                   # noqa: E402
import planted_pnp_lo as PLO               # noqa: E402
import pnp_refine_ref as PR                # noqa: E402
import test_gpu_camera_axes as GA          # noqa: E402  (the map case and the lookup positions: nothing of it is collected from here)
import test_gpu_klt_pnp as KT              # noqa: E402  (the planted pair's keypoints and cloud)
import test_gpu_map as G                   # noqa: E402  (the map suites' window, pose and bars)

X1000 = 1000.0


def _far(pairs, exact=()):
    """pairs: (name, a, b, bar, relative?); exact: (name, a, b) -> (largest distance / bar over the barred fields -- inf when an exact
    field differs --, the field it is in)"""
    for name, a, b in exact:
        if not np.array_equal(np.asarray(a), np.asarray(b)):
            return float("inf"), name + " (exact)"
    best = (0.0, "none")
    for name, a, b, bar, relative in pairs:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if a.shape != b.shape:
            return float("inf"), name + " (shape)"
        with np.errstate(all="ignore"):
            d = np.abs(a - b) / (np.where(b != 0, np.abs(b), 1.0) if relative else 1.0)
        d = float(np.nanmax(d)) if d.size else 0.0
        best = max(best, (d / bar, name))
    return best


# ---- recover_pose -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return CC.mono_scenes()


def _mono_distance(r, m):
    """in the fields test_gpu_planted_mono._check compares: integers, votes4 and the valid set exactly; z1, z2, depth_b, scale_rel to
    1e-12 relative; R, t to 1e-12"""
    return _far([(k, m[k], r[k], 1e-12, True) for k in ("z1", "z2", "depth_b", "scale_rel")] + [(k, m[k], r[k], 1e-12, False) for k in ("R", "t")],
                [(k, m[k], r[k]) for k in ("flags", "winner", "n_depth", "n_shared", "votes4", "valid")])


@pytest.mark.parametrize("name", list(CC.MONO_VOTES) + ["gate", "shared_depth", "n1025"])
def test_recover_pose_cases(scenes, name):
    s = scenes[name]
    r = ref.recover_pose(*CC.mono_args(s, CC.K_640))
    print("%s: n %d, votes %s, winner %d, n_depth %d, n_shared %d, scale_rel %.6g" % (name, len(s["p1"]), list(r["votes4"]), r["winner"], r["n_depth"],
                                                                                    r["n_shared"], r["scale_rel"]))
    assert r["flags"] == 0
    assert len(s["p1"]) <= 300 or name == "n1025"
    if "counts4" in s:                                  # all four chirality candidates voted on, with planted_mono's margin on every sign test
        assert list(r["votes4"]) == list(s["counts4"]) and all(r["votes4"])
        cls, safe = PM.classes(s["E"], s["p1"], s["p2"], CC.K_640)
        assert safe.all() and (cls >= 0).all()
    if name.startswith("winner"):
        assert r["winner"] == int(name[-1]) and r["n_depth"] == max(s["counts4"])
    if name == "tie":
        tr1, tr2 = PM.traces(s["E"])
        assert PM.tie_arms(s["counts4"], tr1, tr2) and r["winner"] == (0 if tr1 >= tr2 else 2)
    if name == "gate":                                  # inliers on both sides, none within 1 % of the gate
        rel = s["sin2"] / PM.GATE - 1.0
        assert (rel > 0.01).sum() >= 5 and (rel < -0.01).sum() >= 5 and (np.abs(rel) > 0.01).all()
        assert 4 < r["n_depth"] < 20 and np.array_equal(r["valid"], s["sin2"] >= PM.GATE)
    if name == "shared_depth":
        assert r["n_depth"] == 50 and 30 <= r["n_shared"] < 50 and r["scale_rel"] > 0
    if name == "n1025":
        assert len(s["p1"]) == 1025 > 1024
    worst = (float("inf"), "")
    for mname, Km in CC.mutants(CC.K_640, 640, 480):
        d = _mono_distance(r, ref.recover_pose(*CC.mono_args(s, Km)))
        print("    %-10s %.3g x the bar, in %s" % (mname, d[0], d[1]))
        assert d[0] >= X1000, (name, mname, d)
        worst = min(worst, d)
    print("    smallest mutant distance: %.3g x the bar (%s)" % worst)


# ---- mono_pose_pair -----------------------------------------------------------------------------------------------------------------------------
def test_mono_pose_pair_case(oracle):
    """the CPU chain of the fused finish on planted_mono's "eight" frames: the oracle's ORB, kNN-2 and ratio test, its eight-point RANSAC
    under the camera, the restated pose tail.  The device test compares the fused step with the composed device chain bit for bit, so
    every field is exact: a mutant must change E or the tail's record."""
    seed, M_want = PM.FINISH_SEEDS["eight"]
    a, b = PM.finish_frames(seed)
    ka, kb = oracle.orb_detect_and_compute(a, None, 2000), oracle.orb_detect_and_compute(b, None, 2000)
    idx, dist = oracle.bf_knn2_hamming(ka["desc"], kb["desc"])
    q, t = oracle.ratio_filter(idx, dist, PM.FINISH_RATIO)
    assert len(q) == M_want == 8
    p1, p2 = ka["xy"][q], kb["xy"][t]

    def chain(K4):
        e = oracle.ransac_essential(p1, p2, K4, *CC.MONO_PAIR_ARGS, solver=8)
        return e, ref.recover_pose(e["E"], p1, p2, list(K4), e["mask"], q, t, len(ka["xy"]), len(kb["xy"]), None, 0.0)
    e, r = chain(CC.K_640)
    print("mono_pose_pair: %d matches, best_count %d @ %d, flags %d, votes %s, winner %d, n_depth %d" % (
        len(q), e["best_count"], e["best_iter"], r["flags"], list(r["votes4"]), r["winner"], r["n_depth"]))
    assert e["best_count"] >= 1 and not (r["flags"] & 1) and r["votes4"].sum() == e["best_count"]      # a live step: a pose was recovered
    for mname, Km in CC.mutants(CC.K_640, 640, 480):
        em, rm = chain(Km)
        fields = [k for k in ("votes4", "winner", "n_depth", "R", "t", "depth_b") if not np.array_equal(rm[k], r[k])]
        fields = (["E"] if not np.array_equal(em["E"], e["E"]) else []) + fields
        print("    %-10s differs in %s; |E - E'| = %.3g" % (mname, fields, float(np.abs(em["E"] - e["E"]).max())))
        assert fields, mname


# ---- pnp_pair, pnp_pair_window, pnp_pair_lo ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pnp_cases():
    return CC.pnp_cases()


def _pnp_distance(m, mm):
    """in the fields test_gpu_planted_pnp._hold_to_model compares: integers, q, t, mask exactly; Rt to 1e-10; Rt_refined to 1e-9"""
    return _far([("Rt", mm["Rt"], m["Rt"], 1e-10, False), ("Rt_refined", mm["Rt64"], m["Rt64"], 1e-9, False)],
                [(k, mm[k], m[k]) for k in ("M", "n", "best_iter", "best_count", "status", "steps", "q", "t", "mask")])


@pytest.mark.parametrize("key", ("M65", "M300", "window"))
def test_pnp_cases(oracle, pnp_cases, key):
    c = pnp_cases[key]
    assert c.K4 == CC.K_640 and PP.PnpCase.K4 == PP.K4 != c.K4
    m = c.model(oracle)
    moved = float(np.abs(m["Rt64"] - m["Rt"]).max())
    to_planted = float(np.abs(m["Rt64"] - PP.planted_Rt()).max())
    print("%s: (nq, M, n) = (%d, %d, %d), best %d @ %d, refit %d / %d moves the winner by %.2e, ends %.2e from the planted pose; float64 | strided | "
          "longdouble sums apart by %.1e" % (c.name, c.nq, m["M"], m["n"], m["best_count"], m["best_iter"], m["status"], m["steps"], moved, to_planted,
                                             max(float(np.abs(m["Rt64"] - m["Rt_strided"]).max()), float(np.abs(m["Rt64"] - m["Rt_ld"]).max()))))
    # the planted PnP model's own checks: the refit ran all its steps, the winner holds most of the planted inliers and only few others,
    # the three summation orders agree far inside the bar
    assert (m["status"], m["steps"]) == (0, 3) and moved > 1e-6 and to_planted < 2e-2
    planted = np.isin(m["q"], c.q0[c.inl_pos])
    assert m["mask"][planted].sum() >= 0.8 * planted.sum() and m["best_count"] >= 6
    assert max(float(np.abs(m["Rt64"] - m["Rt_strided"]).max()), float(np.abs(m["Rt64"] - m["Rt_ld"]).max())) <= 1e-11
    if key == "M65":
        assert m["M"] == 65 and m["n"] > 64
    if key == "M300":
        assert m["M"] == 300 and m["n"] > 256
    if key == "window":                                 # the window removes matches the plain matcher keeps (the partners that lie outside it)
        assert 65 < m["M"] < 300 and planted.sum() >= 150
    worst = (float("inf"), "")
    for mname, Km in CC.mutants(CC.K_640, 640, 480):
        d = _pnp_distance(m, CC.with_camera(c, Km).model(oracle))
        print("    %-10s %.3g x the bar, in %s" % (mname, d[0], d[1]))
        assert d[0] >= X1000, (key, mname, d)
        worst = min(worst, d)
    print("    smallest mutant distance: %.3g x the bar (%s)" % worst)


def test_pnp_lo_case(oracle, pnp_cases):
    c = pnp_cases["lo"]
    rounds, steps = CC.LO_RUN
    m, lm = c.model(oracle), PLO.lo_model(c, oracle, rounds, steps)
    supports = [int(S.sum()) for _, S in lm["trace"]]
    print("%s: n %d, winner %d -> %d rounds, supports %s, status %d, margin %.2e" % (c.name, m["n"], m["best_count"], lm["rounds"], supports, lm["status"],
                                                                                    lm["margin"]))
    assert PLO.admitted(lm) and lm["margin"] >= PLO.MARGIN
    assert m["n"] > 256 and (lm["rounds"], lm["status"]) == (rounds, 0)
    # the re-selection changes the inlier set: round 1's set is not the winner's, and the set the step returns is not the winner's either
    assert not np.array_equal(lm["trace"][0][1], m["mask"]) and not np.array_equal(lm["mask"], m["mask"])
    worst = (float("inf"), "")
    for mname, Km in CC.mutants(CC.K_640, 640, 480):
        cm = CC.with_camera(c, Km)
        mm, lmm = cm.model(oracle), PLO.lo_model(cm, oracle, rounds, steps)
        d = _far([("Rt", mm["Rt"], m["Rt"], 1e-10, False), ("LO pose", lmm["Rt"], lm["Rt"], 1e-9, False)],
                 [("best", (mm["best_iter"], mm["best_count"]), (m["best_iter"], m["best_count"])), ("mask", lmm["mask"], lm["mask"]),
                  ("rounds, support", (lmm["rounds"], lmm["support"]), (lm["rounds"], lm["support"]))])
        print("    %-10s %.3g x the bar, in %s" % (mname, d[0], d[1]))
        assert d[0] >= X1000, (mname, d)
        worst = min(worst, d)
    print("    smallest mutant distance: %.3g x the bar (%s)" % worst)


# ---- klt_pnp_pair -----------------------------------------------------------------------------------------------------------------------------
def test_klt_pnp_case(oracle):
    """the CPU chain of the planted pair (the restatement's tracks, the planted cloud, the oracle's RANSAC, the float64 refit).  The device
    test holds the fused step to the composed device chain bit for bit: every field is exact."""
    c = CC.KLT_CASE
    a, b = C.smooth_pair(KT.W, KT.H)
    xy, special = KT._keypoints(c["n"], None)
    cloud = KT._cloud(xy, None, special, c["K4"])
    xy_b, st, _ = K.track(a, b, xy, win=21, levels=3, fb=1.0)
    idx = np.nonzero(st == 0)[0]
    ok = np.isfinite(cloud[idx]).all(axis=1)
    idx = idx[ok]
    X, uv = np.ascontiguousarray(cloud[idx]), np.ascontiguousarray(xy_b[idx])

    def chain(K4):
        r = oracle.ransac_pnp(X, uv, K4, 256, 1.5, 4321)
        Rt = np.array(r["Rt"]).reshape(3, 4)
        return r, Rt, PR.refine(Rt, X, uv, K4, r["mask"], c["refine"])
    r, Rt, (Rt64, status, steps) = chain(c["K4"])
    print("%s: %d keypoints, %d tracked, n %d, best %d @ %d, refit %d / %d moves the winner by %.2e" % (
        c["name"], c["n"], int((st == 0).sum()), len(idx), r["best_count"], r["best_iter"], status, steps, float(np.abs(Rt64 - Rt).max())))
    # test_gpu_klt_pnp's admission and planted properties: a real consensus, flat-rectangle points, tracks dropped by the 3-D lookup
    assert r["best_count"] >= 0.8 * len(idx) and (status, steps) == (0, c["refine"]) and len(idx) >= 6
    assert (st & 1).any() and (st == 0).sum() >= 30 and len(idx) < (st == 0).sum()
    for mname, Km in CC.mutants(c["K4"], KT.W, KT.H):
        rm, Rtm, (Rt64m, sm, km) = chain(Km)
        d = float(np.abs(Rtm - Rt).max()), float(np.abs(Rt64m - Rt64).max())
        print("    %-10s best %d @ %d; Rt moves by %.3g, Rt_refined by %.3g" % (mname, rm["best_count"], rm["best_iter"], d[0], d[1]))
        assert not np.array_equal(Rtm, Rt) and not np.array_equal(Rt64m, Rt64) and min(d) >= X1000 * 1e-9


# ---- map_view, track_map ------------------------------------------------------------------------------------------------------------------------
def test_map_cases(oracle):
    scene, kind, pose, frame = GA.map_inputs()
    view, rec, _ = GA.map_model(oracle, CC.K_704)
    n = len(scene["xyz"])
    vis = np.zeros(n, bool)
    vis[view["src"]] = True
    counts = {k: (int(vis[kind == i].sum()), int((kind == i).sum())) for i, k in enumerate(CC.MAP_KINDS)}
    print("map: %d landmarks, %d visible; visible / planted per kind: %s" % (n, vis.sum(), counts))
    assert n <= 220
    for k, (v, total) in counts.items():                # inside, and inside | outside each of the four edges, beyond | before z_min, behind
        assert total >= 5 and v == (total if k in ("inside", "near_in") or k.endswith("_in") else 0), (k, v, total)
    # no landmark sits on a bound: the nearest is a good fraction of a pixel away (the view is compared bit for bit, its decisions included)
    u, v = view["xy"][:, 0].astype(np.float64), view["xy"][:, 1].astype(np.float64)
    assert min(u.min(), v.min(), (G.CROP[0] - 1 - u).min(), (G.CROP[1] - 1 - v).min()) > 0.5
    print("track_map: decision %d, vis %d, M %d, n %d, best %d @ %d, refit %d / %d, counts6 %s" % (
        rec["decision"], rec["view"][1], rec["matches"], rec["n"], rec["best_count"], rec["best_iter"], rec["refine_status"], rec["refine_steps"],
        list(rec["update"])))
    assert rec["decision"] == 0 and rec["matches"] >= GA.MAP_M - 5 and rec["best_count"] >= 0.5 * rec["n"]
    assert (rec["refine_status"], rec["refine_steps"]) == (0, GA.MAP_REFINE) and rec["update_flags"] == 0 and (rec["update"] >= 0).all()
    worst = (float("inf"), "")
    for mname, Km in CC.mutants(CC.K_704, G.W, G.H):
        vm, rm, _ = GA.map_model(oracle, Km)
        same_rows = vm["xy"].shape == view["xy"].shape and np.array_equal(G._bits(vm["xy"]), G._bits(view["xy"]))
        moved = int((G._bits(vm["xy"]) != G._bits(view["xy"])).any(1).sum()) if vm["xy"].shape == view["xy"].shape else -1
        d = _far([("Rt", rm["Rt"], rec["Rt"], G.BAR_RT, False), ("Rt_refined", rm["Rt_refined"], rec["Rt_refined"], 1e-9, False),
                  ("c_T_w", rm["c_T_w"], rec["c_T_w"], 1e-9, False)],
                 [(k, rm[k], rec[k]) for k in ("decision", "matches", "n", "best_iter", "best_count")] + [("view", tuple(rm["view"]), tuple(rec["view"]))])
        print("    %-10s view: %d visible, %d keypoints move; step: %.3g x the bar, in %s" % (mname, len(vm["src"]), moved, d[0], d[1]))
        assert not same_rows, mname                    # the view is exact: another value of kp_xy
        assert d[0] >= X1000, (mname, d)
        worst = min(worst, d)
    print("    smallest mutant distance of the step: %.3g x the bar (%s)" % worst)


# ---- direct_align -------------------------------------------------------------------------------------------------------------------------------
GENERIC_DIRECT = [c for c in DC.CASES if c.opt.get("rig") == "generic"]


@pytest.mark.parametrize("case", GENERIC_DIRECT, ids=lambda c: c.name)
def test_direct_cases(case):
    """the regime and the margin of these cases are test_direct_ref.py's (they are members of direct_cases.CASES); here: the rig is
    generic, and every mutant moves the final pose by at least 1000 x the 1e-9 it is held to on the device"""
    A, B, disp, Q, K4, Rt0, _ = case.build()
    assert abs(K4[0] / K4[1] - 1) >= 0.05 and (K4[2], K4[3]) != (-Q[0, 3], -Q[1, 3]) and Q[3, 3] != 0 and Q[3, 2] != 0
    assert np.count_nonzero(Q) == 7                     # the five-entry form (and the two ones): the alignment reads no other entry
    r = DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **case.kw)
    assert r["status"] == 0 and r["margin"] >= DC.MARGIN
    worst = (float("inf"), "")
    for mname, Qm, Km in CC.direct_mutants(Q, K4, case.w, case.h):
        m = DR.align(A, B, disp, Qm, Km, Rt0, roi=case.roi, **case.kw)
        d = _far([("pose", m["Rt"], r["Rt"], 1e-9, False)], [(k, m[k], r[k]) for k in ("status", "iters_done", "s", "selected", "n_first", "n_last", "count")])
        print("%-20s %-10s pose moved by %.3g (%.3g x the bar, in %s)" % (case.name, mname, float(np.abs(m["Rt"] - r["Rt"]).max()), d[0], d[1]))
        assert d[0] >= X1000, (case.name, mname, d)
        worst = min(worst, d)
    print("    smallest mutant distance: %.3g x the bar (%s)" % worst)


# ---- reproject_to_3d, points3d_at ---------------------------------------------------------------------------------------------------------------
def _definition(Q, x, y, d):
    """float64 Q v / (Q v)[3] for v = (x, y, d, 1) -> (points (..., 3), the magnitude of the terms of each component over |w|)"""
    v = np.stack(np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(d, np.float64), 1.0), -1)
    hg = v @ np.asarray(Q, np.float64).T
    mag = np.abs(v) @ np.abs(np.asarray(Q, np.float64)).T
    return hg[..., :3] / hg[..., 3:], (mag[..., :3] + np.abs(hg[..., :3]) * (mag[..., 3:] / np.abs(hg[..., 3:]))) / np.abs(hg[..., 3:])


@pytest.mark.parametrize("w,h", CC.REPROJECT_SHAPES)
def test_reprojection_oracle_is_the_full_matrix_product(oracle, w, h):
    """The oracle against float64 Q v / (Q v)[3], per component.  Its arithmetic: the float64 sums, ONE rounding of each numerator to
    float32, a float64 product with 1 / w, ONE rounding of the product to float32 -- two float32 roundings, each at most 2^-24
    relative, so 2^-23 of the component; the float64 sums add at most 8 x 2^-53 of their terms' magnitudes (four products, three
    additions, the reciprocal), which matters only where a component cancels."""
    Q, disp = CC.full_Q(w, h), CC.disparity(w, h)
    assert np.count_nonzero(Q) == 16 and Q[3, 0] != 0 and Q[3, 1] != 0 and (disp == 0).any() and (disp < 0).any()
    y, x = np.mgrid[0:h, 0:w]
    want, mag = _definition(Q, x, y, disp)
    got = oracle.reproject_to_3d(disp, Q).astype(np.float64)
    bound = 2.0 ** -23 * np.abs(want) + 8 * 2.0 ** -53 * mag
    worst = float((np.abs(got - want) / bound).max())
    print("reproject %d x %d: largest |oracle - definition| = %.3g of its bound (%.3g relative)" % (w, h, worst, float((np.abs(got - want) / np.abs(want)).max())))
    assert np.isfinite(want).all() and worst <= 1.0
    # every entry of Q matters, bit for bit (the device is held to the oracle in its bits)
    bits = oracle.reproject_to_3d(disp, Q).view(np.uint32)
    fewest = min((int((oracle.reproject_to_3d(disp, Qm).view(np.uint32) != bits).sum()), mname) for mname, Qm in CC.q_mutants(Q))
    print("    the mutant that changes the fewest values: %s (%d of %d)" % (fewest[1], fewest[0], bits.size))
    assert fewest[0] > 0


@pytest.mark.parametrize("w,h", CC.REPROJECT_SHAPES)
def test_lookup_oracle_is_the_bilinear_mean_of_the_product(oracle, w, h):
    """oracle.points3d_at against the float64 bilinear mean of the float64 points of the taps that exist (every tap is finite under
    this Q).  Its arithmetic on float32 taps: four weights rounded to float32, four products and three additions in float32, the
    denominator rounded, one division -- 14 float32 roundings on top of the taps' own 2 (above), none cancelling beyond the taps'
    magnitude: 16 x 2^-24 of the largest tap component."""
    Q, disp = CC.full_Q(w, h), CC.disparity(w, h)
    disp16 = np.rint(16.0 * disp).astype(np.int16)
    xy = GA.lookup_positions(w, h)
    got, st = oracle.points3d_at(disp16, Q, (0, 0, 1 << 20, 1 << 20), xy)
    assert (st == 0).all() and len(xy) >= 60
    worst = 0.0
    for (px, py), g in zip(xy.astype(np.float64), got.astype(np.float64)):
        fx, fy = int(px), int(py)
        rx, ry = px - fx, py - fy
        num, den, big = np.zeros(3), 0.0, np.zeros(3)
        for tx, ty, wt in ((fx, fy, (1 - rx) * (1 - ry)), (fx, fy + 1, (1 - rx) * ry), (fx + 1, fy, rx * (1 - ry)), (fx + 1, fy + 1, rx * ry)):
            if tx >= w or ty >= h:
                continue
            p, _ = _definition(Q, tx, ty, disp16[ty, tx] / 16.0)
            num, den, big = num + wt * p, den + wt, np.maximum(big, np.abs(p))
        worst = max(worst, float((np.abs(g - num / den) / (16 * 2.0 ** -24 * big)).max()))
    print("points3d_at %d x %d: %d lookups, largest |oracle - definition| = %.3g of its bound" % (w, h, len(xy), worst))
    assert worst <= 1.0
    bits = got.view(np.uint32)
    fewest = min((int((oracle.points3d_at(disp16, Qm, (0, 0, 1 << 20, 1 << 20), xy)[0].view(np.uint32) != bits).sum()), mname) for mname, Qm in CC.q_mutants(Q))
    print("    the mutant that changes the fewest values: %s (%d of %d)" % (fewest[1], fewest[0], bits.size))
    assert fewest[0] > 0
