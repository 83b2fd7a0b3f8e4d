"""Scenes and cases for the definition tests of the RANSAC fronts (tests/test_score_ref.py on the CPU oracle,
tests/test_gpu_ransac_definitions.py on the device).  numpy only.

ESS_CASES / PNP_CASES are a subset of n x iters x thr x K4 x scene that meets every value of every axis:
    n       8 (6 for the five-point solver, 4 for PnP), 63, 64, 65, 3000: one wave scores one hypothesis, 64 points a trip
    iters   1, 4, 5, 300: four hypotheses a block
    thr     0.1, 1.0, 5.0
    K4      640 x 480, 1920 x 1080, 3840 x 2160 and a camera with fx != fy and the principal point in the image corner
    motion  "mixed" t = (0.05, 0.01, -0.25), "forward" (0, 0, 0.3): the epipole inside the image, "sideways" (0.3, 0, 0)
Essential scenes draw the first view's pixels uniformly over the image (some land within a few pixels of the epipole), with
0.3 px noise and 25 % outliers.  PnP scenes have depths from 1 m to 400 m; "behind" moves points behind the camera (mirrored through
its centre, so that their pixel still fits and only the depth rule excludes them) or onto its plane; "offset" shifts the 3-D points
(and the pose with them) 1e4 m from the origin."""
import numpy as np

K_VGA = (400.0, 400.0, 320.0, 240.0)
K_HD = (1050.0, 1050.0, 960.0, 540.0)
K_4K = (2100.0, 2100.0, 1920.0, 1080.0)
K_SKEW = (700.0, 650.0, 0.0, 0.0)
IMAGE = {K_VGA: (640, 480), K_HD: (1920, 1080), K_4K: (3840, 2160), K_SKEW: (640, 480)}
MOTION = {"mixed": (0.05, 0.01, -0.25), "forward": (0.0, 0.0, 0.3), "sideways": (0.3, 0.0, 0.0)}
NOISE, OUTLIERS = 0.3, 0.25
SEED = 4321                                # the RANSAC seed of every case


def rotation(ang=0.03):
    return np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])


def project(Y, K4):
    return np.stack([K4[0] * Y[:, 0] / Y[:, 2] + K4[2], K4[1] * Y[:, 1] / Y[:, 2] + K4[3]], 1)


def backproject(p, Z, K4):
    return np.stack([(p[:, 0] - K4[2]) / K4[0] * Z, (p[:, 1] - K4[3]) / K4[1] * Z, Z], 1)


def essential_scene(n, K4, motion, seed, noise=NOISE, outliers=OUTLIERS, zmin=2.0, zmax=40.0):
    """-> dict(p1, p2 float32 (n, 2), K4, R, t, out: the outliers' indices)"""
    rng = np.random.default_rng([3, seed, n])
    w, h = IMAGE[K4]
    R, t = rotation(), np.array(MOTION[motion], np.float64)
    while True:
        p1 = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
        X = backproject(p1, np.exp(rng.uniform(np.log(zmin), np.log(zmax), n)), K4)
        Y = X @ R.T + t
        if (Y[:, 2] > 0.5).all():
            break
    p2 = project(Y, K4)
    p1, p2 = p1 + rng.normal(0, noise, (n, 2)), p2 + rng.normal(0, noise, (n, 2))
    out = np.sort(rng.choice(n, int(n * outliers), replace=False))
    p2[out] += rng.uniform(-80, 80, (len(out), 2))
    return dict(p1=np.ascontiguousarray(p1, np.float32), p2=np.ascontiguousarray(p2, np.float32), K4=K4, R=R, t=t, out=out)


def pnp_scene(n, K4, seed, behind=0, offset=0.0, noise=NOISE, outliers=OUTLIERS, zmin=1.0, zmax=400.0):
    """-> dict(X float32 (n, 3), uv float32 (n, 2), K4, Rt 3x4, out, behind: the indices moved behind the camera or onto its plane)"""
    rng = np.random.default_rng([5, seed, n])
    w, h = IMAGE[K4]
    R, t = rotation(), np.array(MOTION["mixed"], np.float64)
    p = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    X = backproject(p, np.exp(rng.uniform(np.log(zmin), np.log(zmax), n)), K4)
    Y = X @ R.T + t
    uv = project(Y, K4) + rng.normal(0, noise, (n, 2))
    out = np.sort(rng.choice(n, int(n * outliers), replace=False))
    uv[out] += rng.uniform(-60, 60, (len(out), 2))
    moved = np.sort(rng.choice(np.setdiff1d(np.arange(n), out), behind, replace=False)) if behind else np.zeros(0, np.int64)
    for k, i in enumerate(moved):
        Yi = -Y[i] if k % 3 else np.array([Y[i, 0], Y[i, 1], 0.0])      # two in three mirrored, one in three on the camera's plane
        X[i] = R.T @ (Yi - t)
        uv[i] = project(Y[i:i + 1], K4)[0]             # (no noise: a model that fits the scene fits these pixels)
    if offset:
        c = np.array([offset, -offset, offset])
        X, t = X + c, t - R @ c
    return dict(X=np.ascontiguousarray(X, np.float32), uv=np.ascontiguousarray(uv, np.float32), K4=K4, Rt=np.c_[R, t], out=out, behind=moved)


# (n, iters, thr, K4, motion); the five-point solver runs the same cases with n = 6 in place of 8
ESS_CASES = [(8, 1, 1.0, K_VGA, "mixed"), (63, 4, 5.0, K_HD, "forward"), (64, 5, 1.0, K_4K, "sideways"), (65, 300, 0.1, K_SKEW, "mixed"),
             (3000, 300, 0.1, K_4K, "forward"), (3000, 300, 5.0, K_VGA, "sideways"), (3000, 5, 1.0, K_HD, "forward"),
             (3000, 4, 0.1, K_HD, "mixed")]
# (n, iters, thr, K4, behind, offset)
PNP_CASES = [(4, 1, 1.0, K_SKEW, 0, 0.0), (63, 4, 5.0, K_VGA, 6, 0.0), (64, 5, 1.0, K_4K, 6, 0.0), (65, 300, 0.1, K_SKEW, 6, 0.0),
             (3000, 300, 0.1, K_4K, 60, 0.0), (3000, 300, 5.0, K_SKEW, 60, 0.0), (3000, 5, 1.0, K_HD, 60, 0.0)]
PNP_OFFSET_CASE = (3000, 300, 1.0, K_HD, 60, 1e4)
CAP = 0.02                                 # the largest undecidable share of a scene
# scenes under which so few hypotheses still hold a good one (found by a loop over 0 .. 11): only a model that fits makes the
# mirrored points inliers of the definition without its depth rule (tests/test_score_ref.py, the power of the test)
PNP_SCENE_SEEDS = {(63, 4): 1}


def ess_case_scene(case, solver):
    n, iters, thr, K4, motion = case
    n = 6 if (n == 8 and solver == 5) else n
    return essential_scene(n, K4, motion, seed=ESS_CASES.index(case)), n, iters, thr


def pnp_case_scene(case):
    n, iters, thr, K4, behind, offset = case
    return pnp_scene(n, K4, seed=PNP_SCENE_SEEDS.get((n, iters), 17 + n + iters), behind=behind, offset=offset), n, iters, thr


def case_id(case):
    k = {K_VGA: "vga", K_HD: "hd", K_4K: "4k", K_SKEW: "skew"}[case[3]]
    return "n%d-it%d-thr%g-%s-%s" % (case[0], case[1], case[2], k, "-".join(str(v) for v in case[4:]))


def winner_rule(r):
    """best_count == mask.sum() == counts[best_iter], and best_iter is the lowest index that holds the maximum"""
    counts = np.asarray(r["counts"])
    assert r["best_count"] == int(np.asarray(r["mask"]).sum()) == int(counts[r["best_iter"]]), (r["best_count"], int(r["mask"].sum()), int(counts[r["best_iter"]]))
    assert r["best_iter"] == int(np.argmax(counts)) and r["best_count"] == int(counts.max())


# ---- the hypothesis generators at the sample sizes where every hypothesis must be exact ---------------------------------------
GEN_ITERS, GEN_SEEDS, GEN_THR = 256, 20, 1.0
GEN_K4 = K_HD


def exact_scene(n, seed, K4=GEN_K4, zmin=4.0, zmax=40.0):
    """noise-free float32 pixels of n points in general position -> dict(p1, p2, X, K4, R, t, Rt)"""
    rng = np.random.default_rng([7, seed, n])
    w, h = IMAGE[K4]
    R, t = rotation(0.03 + 0.002 * seed), np.array(MOTION["mixed"], np.float64) + np.array([0.1, -0.05, 0.0])
    p1 = np.stack([rng.uniform(0.1 * w, 0.9 * w, n), rng.uniform(0.1 * h, 0.9 * h, n)], 1).astype(np.float32)
    X = backproject(p1.astype(np.float64), rng.uniform(zmin, zmax, n), K4).astype(np.float32)
    p1 = project(X.astype(np.float64), K4).astype(np.float32)
    p2 = project(X.astype(np.float64) @ R.T + t, K4).astype(np.float32)
    return dict(p1=p1, p2=p2, X=X, K4=K4, R=R, t=t, Rt=np.c_[R, t])


def normalised(p, K4):
    p = np.asarray(p, np.float32).astype(np.float64)
    return np.stack([(p[:, 0] - K4[2]) / K4[0], (p[:, 1] - K4[3]) / K4[1], np.ones(len(p))], 1)


def algebraic_residuals(E, s):
    """|x2^T E x1| of every point, E at unit Frobenius norm"""
    E = np.asarray(E, np.float64) / np.linalg.norm(E)
    x1, x2 = normalised(s["p1"], s["K4"]), normalised(s["p2"], s["K4"])
    return np.abs(((x2 @ E) * x1).sum(1))


def lapack_eight_point(s):
    """the null vector of the 8 x 9 system by np.linalg.svd, projected to singular values (1, 1, 0)"""
    x1, x2 = normalised(s["p1"], s["K4"]), normalised(s["p2"], s["K4"])
    A = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1], x1[:, 0], x1[:, 1],
                  np.ones(len(x1))], 1)
    e = np.linalg.svd(A)[2][-1].reshape(3, 3)
    Ue, _, Vte = np.linalg.svd(e)
    return Ue @ np.diag([1.0, 1.0, 0.0]) @ Vte


def check_eight_point(r, s):
    """one run of 256 hypotheses on an 8-point scene -> (hypotheses that count 8, residual ratio to LAPACK)"""
    full = int((np.asarray(r["counts"]) == 8).sum())
    assert full >= 254, "%d of %d hypotheses count all eight points" % (full, GEN_ITERS)
    w = np.linalg.svd(r["E"], compute_uv=False)
    assert abs(w[0] - w[1]) / w[0] <= 1e-12 and w[2] / w[0] <= 1e-12, w
    res, ref = float(algebraic_residuals(r["E"], s).max()), float(algebraic_residuals(lapack_eight_point(s), s).max())
    assert res <= 1.05 * ref + 1e-12, "largest residual %.3g, LAPACK %.3g" % (res, ref)
    return full, res / ref if ref > 0 else 1.0


def check_five_point(r, s):
    """-> (|det E|, the cubic constraint's largest entry, hypotheses that count 6) of the winner on a 6-point scene"""
    E = np.asarray(r["E"], np.float64)
    assert abs(np.linalg.norm(E) - 1.0) < 1e-12
    res = algebraic_residuals(E, s)
    assert int((res < 1e-10).sum()) >= 5, res
    det, cubic = abs(np.linalg.det(E)), float(np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())
    assert det < 1e-4 and cubic < 1e-4, (det, cubic)
    assert r["best_count"] == 6
    return det, cubic, int((np.asarray(r["counts"]) == 6).sum())


def check_five_point_over_scenes(dets, cubics):
    """the bars tests/test_oracle_known_answers.py::test_five_point_solutions_satisfy_every_constraint holds the oracle's solutions to"""
    dets, cubics = np.asarray(dets), np.asarray(cubics)
    assert np.median(dets) < 1e-12 and np.mean(dets < 1e-9) > 0.9 and dets.max() < 1e-4, dets
    assert np.median(cubics) < 1e-12 and np.mean(cubics < 1e-9) > 0.9 and cubics.max() < 1e-4, cubics


P3P_K4 = (1024.0, 1024.0, 960.0, 540.0)


def dyadic_pnp_scene(seed):
    """Four points whose float32 coordinates AND float32 pixels are exact under the planted pose: a quarter turn about the optical
    axis, a translation in sixteenths, depths 4 .. 32 m that are powers of two, pixels on the half-pixel grid of a camera with
    f = 1024.  Rounding pixels to float32 moves the pose that three GENERIC points define by 1e-6 at the median and by up to 6e-5
    (first-order sensitivity at depths to 40 m, and the oracle on exact_scene(4, .)): the 1e-6 bar on the pose is held where the
    data carry no rounding, so that what it measures is the solver."""
    rng = np.random.default_rng([11, seed])
    R, t = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.125, -0.0625, -0.25])
    while True:
        z = rng.choice([4.0, 8.0, 16.0, 32.0], 4)
        uv = np.stack([rng.integers(200, 3640, 4) / 2.0, rng.integers(120, 2040, 4) / 2.0], 1)
        if len(set(z)) >= 2 and len(set(uv[:, 0])) == 4 and len(set(uv[:, 1])) == 4:
            break
    Y = np.stack([(uv[:, 0] - P3P_K4[2]) * z / P3P_K4[0], (uv[:, 1] - P3P_K4[3]) * z / P3P_K4[1], z], 1)
    X = (Y - t) @ R                                   # R^T (Y - t)
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X) and np.array_equal(project(X @ R.T + t, P3P_K4), uv)
    return dict(X=X.astype(np.float32), p2=uv.astype(np.float32), K4=P3P_K4, Rt=np.c_[R, t])


def check_p3p(r, s, bar=1e-6):
    """every hypothesis counts all four points -> the distance of Rt from the planted pose, held to `bar` (None: a figure only)"""
    assert (np.asarray(r["counts"]) == 4).all(), "%d of %d hypotheses count all four points" % (int((np.asarray(r["counts"]) == 4).sum()), GEN_ITERS)
    d = float(np.abs(np.asarray(r["Rt"]) - s["Rt"]).max())
    assert bar is None or d <= bar, "Rt is %.3g from the planted pose" % d
    return d


# ---- ties, and a second trip of the block-wide argmax -----------------------------------------------------------------------------
# At n = 8 (6 for the five-point solver, 4 for PnP) every hypothesis sees every point of a noise-free scene, so many hypotheses hold
# the full count and the winner is decided by the tie-break alone; 257 and 1025 hypotheses give a 256-thread and a 1024-thread
# block a second trip through the counts.  The scenes are exact_scene's: TIE_K4 for the stand-alone entries, the small camera
# for the slots of the fused steps.
TIE_ITERS = (257, 1025)
TIE_N = {8: 8, 5: 6, "pnp": 4}             # solver -> n
TIE_SCENE_SEED = 3


def tie_scene(solver, K4=GEN_K4):
    return exact_scene(TIE_N[solver], TIE_SCENE_SEED, K4=K4)


def ties(counts):
    """-> how many hypotheses hold the largest count"""
    counts = np.asarray(counts)
    return int((counts == counts.max()).sum())


def tie_rule(r):
    """winner_rule on a run whose winner the tie-break decided"""
    assert ties(r["counts"]) >= 2, "only one hypothesis holds the largest count %d" % int(np.asarray(r["counts"]).max())
    winner_rule(r)


# ---- the scenes planted into slots for the fused steps ---------------------------------------------------------------------------
FUSED_NQ, FUSED_M, FUSED_ITERS, FUSED_THR, FUSED_RATIO = 230, 200, 300, 1.0, 0.8     # 200 matches: three trips of a wave and a tail


def fused_essential_scene(solver):
    return essential_scene(FUSED_M, K_VGA, "mixed", seed=50 + solver)


def fused_pnp_scene():
    return pnp_scene(FUSED_M, K_VGA, seed=61, behind=6, zmax=60.0)


def nan_scene():
    """65 points of the 1920 x 1080 mixed scene, three of them NaN in both views -> (scene, the three indices)"""
    s = essential_scene(65, K_HD, "mixed", seed=99)
    bad = np.array([0, 31, 64])
    s["p1"][bad] = np.nan
    s["p2"][bad] = np.nan
    return s, bad
