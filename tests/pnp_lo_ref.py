"""numpy restatement of the local-optimisation rounds of the stereo PnP step (include/vo355.h, vo_pnp_pair_lo): test infrastructure.

Inputs: the RANSAC winner Rt_0 (float64 3x4), its mask S_0, the n usable correspondences X / uv (float32), K4, thr (float32),
steps = refine_iters (1 .. 20), rounds R (1 .. 8).  For r = 1 .. R:

    1. (Rt_r, status, _) = pnp_refine_ref.refine(Rt_{r-1}, X, uv, K4, S_{r-1}, steps)       today's arithmetic, unchanged
    2. status != 0 (1: fewer than 6 points in S_{r-1}; -1: a pivot not positive or a value not finite): the round is discarded
       entirely and the loop ends
    3. S_r[i] = the scoring kernels' own test under Rt_r for every i < n: P = K [R | t] rounded to float32 the way k_pnp_hyp forms
       a hypothesis's P, then the division-free float32 test against thr * thr (reproj_inlier of csrc/ransac.hip)

The result is (Rt_c, S_c) of the last completed round c = 0 .. R; status 0 when c >= 1, otherwise the status of round 1 (today's
refinement status for the same inputs).  No early exit, no acceptance test: a function of the inputs alone.  With R = 1 the pose
is pnp_refine_ref.refine's, bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_refine_ref as PR                # noqa: E402
import sparse_stereo_ref as S              # noqa: E402


def form_P(Rt, K4):
    """float32 P (12,) of the float64 pose: (float)(fx Rt[c] + cx Rt[8 + c]), (float)(fy Rt[4 + c] + cy Rt[8 + c]), (float)Rt[8 + c]"""
    Rt = np.asarray(Rt, np.float64).reshape(12)
    fx, fy, cx, cy = (float(v) for v in K4)
    P = np.empty(12, np.float32)
    for c in range(4):
        P[c] = np.float32(fx * Rt[c] + cx * Rt[8 + c])
        P[4 + c] = np.float32(fy * Rt[4 + c] + cy * Rt[8 + c])
        P[8 + c] = np.float32(Rt[8 + c])
    return P


def select(P, X, uv, thr):
    """mask (n,) uint8: reproj_inlier in float32, operation by operation (float32 arrays: numpy contracts nothing)"""
    P = np.asarray(P, np.float32)
    X, uv = np.asarray(X, np.float32).reshape(-1, 3), np.asarray(uv, np.float32).reshape(-1, 2)
    thr2 = np.float32(thr) * np.float32(thr)
    x, y, z, u, v = X[:, 0], X[:, 1], X[:, 2], uv[:, 0], uv[:, 1]
    with np.errstate(all="ignore"):
        xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3]
        yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7]
        zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11]
        du, dv = xc - u * zc, yc - v * zc
        e = du * du + dv * dv
        lim = thr2 * (zc * zc)
        assert e.dtype == np.float32 and lim.dtype == np.float32
        return ((zc > np.float32(0)) & (e < lim)).astype(np.uint8)


def select_margin(P, X, uv, thr):
    """the smallest |e - lim| / lim over the points in front of the camera, in float64 from the float32 P: how far the nearest
    point sits from the threshold (relative, in squared pixels)"""
    P = np.asarray(P, np.float32).astype(np.float64)
    X, uv = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(uv, np.float32).astype(np.float64).reshape(-1, 2)
    thr2 = float(np.float32(thr) * np.float32(thr))
    Y = X @ P.reshape(3, 4)[:, :3].T + P.reshape(3, 4)[:, 3]
    zc = Y[:, 2]
    e = (Y[:, 0] - uv[:, 0] * zc) ** 2 + (Y[:, 1] - uv[:, 1] * zc) ** 2
    lim = thr2 * zc * zc
    ok = zc > 0
    return float((np.abs(e[ok] - lim[ok]) / lim[ok]).min()) if ok.any() else float("inf")


def lo(Rt0, S0, X, uv, K4, thr, steps, rounds, order=None, dtype=np.float64, trace=None, poses=None):
    """-> (Rt 3x4 float64, S uint8 (n,), status, Gauss-Newton steps applied in the completed rounds, rounds completed c).
    order: None (ascending sums) or a function mask -> the inliers' indices in the order to sum them; dtype: the type of the sums
    (pnp_refine_ref.refine).  trace / poses (lists): receive (P float32, S_r) / Rt_r of every completed round."""
    if not (1 <= steps <= 20 and 1 <= rounds <= 8):
        raise ValueError("steps is 1 .. 20 and rounds 1 .. 8")
    Rt = np.array(Rt0, np.float64).reshape(3, 4)
    S = np.asarray(S0, np.uint8).copy()
    X, uv = np.asarray(X, np.float32).reshape(-1, 3), np.asarray(uv, np.float32).reshape(-1, 2)
    status1, c = 0, 0
    for r in range(1, rounds + 1):
        new, status, _ = PR.refine(Rt, X, uv, K4, S, steps, order=None if order is None else order(S), dtype=dtype)
        if r == 1:
            status1 = status
        if status != 0:
            break
        Rt = new
        P = form_P(Rt, K4)
        S = select(P, X, uv, thr)
        c = r
        if trace is not None:
            trace.append((P, S.copy()))
        if poses is not None:
            poses.append(Rt.copy())
    return Rt, S, (0 if c >= 1 else status1), c * steps, c


class LoRefOdometer(S.SparseRefOdometer):
    """SparseRefOdometer whose PnP pose goes through the restated step: pnp_refine steps on the winner's inliers (rounds = 0, the
    odometer of today) or `rounds` local-optimisation rounds.  The decisions are SparseRefOdometer's: "outlier" reads the winner's
    count, the gates see the refitted pose when its status is 0.  memo (optional, shared between instances): the three traced rounds
    of a (pair, parameters) -- a round does not know how many follow, so rounds 1 .. 3 of one run serve every instance."""

    def __init__(self, *a, refine=0, rounds=0, memo=None, **kw):
        super().__init__(*a, pose_method="pnp", **kw)
        self.refine, self.rounds, self.memo = refine, rounds, memo
        self.lo_counts = None

    def try_pair(self, a, b, span):
        q, t = self.matches(a, b, span)
        self.log.append((len(a["xy"]), len(b["xy"]), len(q)))
        if len(q) < self.min_matches:
            self.skip_cause = "matches"
            return None
        X = a["xyz"][q]
        ok = np.isfinite(X).all(axis=1)
        uv = b["xy"][t] + np.array(b["origin"], np.float32)
        if ok.sum() < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        Q = self.Q
        K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
        key = (id(a), id(b), span, self.pnp, self.refine, self.cross_check, self.match_window)
        got = None if self.memo is None else self.memo.get(key)
        if got is None:
            X, uv = np.ascontiguousarray(X[ok]), np.ascontiguousarray(uv[ok])
            r = self.O.ransac_pnp(X, uv, K4, *self.pnp)
            Rt0 = np.asarray(r["Rt"], np.float64).reshape(3, 4)
            poses = [(Rt0, int(r["best_count"]))]
            if self.refine > 0 and r["best_count"] >= self.min_matches:
                tr, Rts = [], []
                lo(Rt0, r["mask"], X, uv, K4, self.pnp[1], self.refine, 3 if self.memo is not None else max(self.rounds, 1), trace=tr, poses=Rts)
                poses += [(Rt, int(Sm.sum())) for Rt, (_, Sm) in zip(Rts, tr)]
            got = (int(r["best_count"]), poses)
            if self.memo is not None:
                self.memo[key] = got
        best_count, poses = got
        if best_count < self.min_matches:
            self.skip_cause = "outlier"
            return None
        c = min(max(self.rounds, 1) if self.refine > 0 else 0, len(poses) - 1)
        Rt, support = poses[c]
        self.lo_counts = (c if self.rounds > 0 else 0, support)
        return self._gate(np.vstack([Rt, [0, 0, 0, 1]]))
