"""Inputs and plain references for the planted-slot tests of the fused pose step (k_pose_prep -> k_pose_cons_bits -> k_pose_solve
in csrc/geom.hip).  No GPU in here.

A case is two keypoint sets (descriptors + 3-D points) built so that the step meets a chosen (nq, M) and a chosen geometry:

    descriptors(nq, M, ...)      train descriptors are random; a query that must match is a copy of its partner (a few bits
                                 flipped), the rest are random
    matches(dq, dt, ratio)       the matches the step must find: numpy brute-force Hamming (unpackbits), lower index on ties, the
                                 float32 ratio test -- computed, never assumed from the construction
    GEOMETRY[name](n, rng)       -> (pa, pb) float32 (n, 3): the 3-D points of the n matches in match order
    np_fit(src, dst)             high-precision Umeyama: means in longdouble, covariance in float64, np.linalg.svd
    model(case)                  what the fused step must return: matches -> oracle.rigid_clique -> np_fit / np.median outlier rule
    restated(pa, pb, ...)        tests/pose_fit_ref.py (the kernel's own summation order) for n <= 1024

RATIO, RIGIDITY, OUTLIER, MIN_MATCHES are the defaults of every case."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_fit_ref as PF                  # noqa: E402

RATIO, RIGIDITY, OUTLIER, MIN_MATCHES = 0.8, 0.1, 0.02, 10
THR32 = np.float32(RIGIDITY)               # the threshold as the consistency rows compare it


# ---------------------------------------------------------------------------------------------- descriptors and matches
def hamming(a, b):
    """(na, 32) x (nb, 32) uint8 -> (na, nb) int32 Hamming distances"""
    A = np.unpackbits(np.asarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    B = np.unpackbits(np.asarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    d = A.sum(1)[:, None] + B.sum(1)[None, :] - 2.0 * (A @ B.T)        # integers below 2^24: exact in float32
    return np.rint(d).astype(np.int32)


def knn2(dq, dt):
    """brute-force 2 nearest train descriptors of every query, lower index on equal distance -> (idx (nq, 2), dist (nq, 2))"""
    d = hamming(dq, dt)
    nq = len(d)
    rows = np.arange(nq)
    i0 = d.argmin(1)                      # (first occurrence = lowest index)
    d0 = d[rows, i0]
    d[rows, i0] = np.iinfo(np.int32).max
    i1 = d.argmin(1)
    d1 = d[rows, i1]
    return np.stack([i0, i1], 1).astype(np.int32), np.stack([d0, d1], 1).astype(np.int32)


def ratio_test(idx, dist, ratio):
    a = dist[:, 0].astype(np.float32).astype(np.float64)
    b = dist[:, 1].astype(np.float32).astype(np.float64)
    keep = (idx[:, 1] >= 0) & (a < ratio * b)
    return np.nonzero(keep)[0].astype(np.int32), idx[keep, 0].astype(np.int32)


def matches(dq, dt, ratio=RATIO):
    if len(dq) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    idx, dist = knn2(dq, dt)
    return ratio_test(idx, dist, ratio)


def descriptors(nq, M, rng, extra_train=7, flips=2):
    """-> (dq (nq, 32), dt (nt, 32), q (M,), t (M,)): M of the nq queries, spread over the set, are copies of distinct train
    descriptors with up to `flips` bits flipped"""
    nt = max(M + extra_train, 2)
    dt = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    dq = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    q = np.sort(rng.choice(nq, M, replace=False)).astype(np.int32)
    t = rng.permutation(nt)[:M].astype(np.int32)
    dq[q] = dt[t]
    for k in range(M):
        for bit in rng.choice(256, int(rng.integers(0, flips + 1)), replace=False):
            dq[q[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
    return dq, dt, q, t


# ---------------------------------------------------------------------------------------------- geometry
def _motion(angle=0.05, t=(0.05, -0.02, 0.3)):
    ax = np.array([0.3, 1.0, 0.2]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K), np.array(t, np.float64)


def _cloud(n, rng):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(2, 10, n)], 1)


def _move(P, rng, noise=1e-3):
    R, t = _motion()
    return P @ R.T + t + rng.normal(0, noise, P.shape)


def g_rigid(n, rng):
    """every pair rigid (1 mm noise)"""
    P = _cloud(n, rng)
    return P, _move(P, rng)


def g_rigid_out(n, rng):
    """rigid inliers plus gross outliers (one in five, far away: consistent with almost nothing)"""
    P = _cloud(n, rng)
    Q = _move(P, rng)
    out = rng.random(n) < 0.2
    if n >= 5:
        out[:5] = [False, True, False, False, True]
    Q[out] = rng.uniform(-100, 100, (int(out.sum()), 3))
    return P, Q


def g_soft(n, rng):
    """rigid inliers plus pairs displaced by 0.5: what the outlier pass (not the clique filter) has to remove"""
    P = _cloud(n, rng)
    Q = _move(P, rng)
    k = max(1, n // 7)
    sel = rng.choice(n, k, replace=False)
    d = rng.normal(0, 1, (k, 3))
    Q[sel] += 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return P, Q


def g_two_groups(n, rng):
    """two interleaved rigid groups of equal size under different motions: every row count ties, the lowest index wins"""
    n2 = n - (n & 1)
    P = _cloud(n, rng)
    Q = _move(P, rng, noise=0.0)
    Q[1:n2:2] += np.array([100.0, 0.0, 0.0])
    if n & 1:
        Q[n - 1] = [500.0, 500.0, 500.0]          # (an odd one out: consistent with nothing)
    return P, Q


def g_threshold(n, rng):
    """pair distances exactly AT the rigidity threshold and one float32 ulp to either side: all previous points coincide, the current
    ones lie on the x axis at 0, thr - ulp, thr, thr + ulp, 2 thr (every difference of two of them is exact in float32)"""
    lo, hi = np.nextafter(THR32, np.float32(0)), np.nextafter(THR32, np.float32(1))
    vals = np.array([0, lo, THR32, hi, np.float32(2) * THR32], np.float32)
    P = np.zeros((n, 3), np.float32)
    Q = np.zeros((n, 3), np.float32)
    Q[:, 0] = vals[(np.arange(n) * 3) % 5]
    return P, Q


def g_clique_one(n, rng):
    """no two pairs consistent: a clique of one"""
    P = np.zeros((n, 3), np.float32)
    Q = np.zeros((n, 3), np.float32)
    Q[:, 0] = np.arange(n, dtype=np.float32)
    return P, Q


def g_dup(n, rng):
    """every pair twice (tied residuals), softly displaced ones among them"""
    h = (n + 1) // 2
    P, Q = g_soft(h, rng)
    P, Q = P.astype(np.float32), Q.astype(np.float32)
    return np.concatenate([P, P[:n - h]]), np.concatenate([Q, Q[:n - h]])


def g_planar_frontal(n, rng):
    P = _cloud(n, rng)
    P[:, 2] = 5.0
    R, t = _motion()
    Q = P @ R.T + t
    return P, Q


def g_planar_tilted(n, rng):
    P = _cloud(n, rng)
    P[:, 2] = 5.0 + 0.5 * P[:, 0] - 0.25 * P[:, 1]
    R, t = _motion()
    return P, P @ R.T + t


def g_near_planar(n, rng):
    P = _cloud(n, rng)
    P[:, 2] = 5.0 + rng.uniform(-1e-4, 1e-4, n)
    return P, _move(P, rng, noise=1e-5)


def g_mirrored(n, rng):
    """the target is a mirror image: the best orthogonal fit is a reflection, the fit must return the best ROTATION"""
    P = _cloud(n, rng)
    Q = _move(P, rng)
    Q[:, 2] = 12.0 - Q[:, 2]
    return P, Q


def g_x8(n, rng):
    P, Q = g_rigid(n, rng)
    return 8.0 * P, 8.0 * Q


def g_motion_1e6(n, rng):
    P = _cloud(n, rng)
    return P, P + np.array([1e-6, -1e-6, 1e-6])


def g_identical(n, rng):
    """all points identical: the covariance is exactly zero (rc = -2)"""
    return np.tile(np.float32([0.5, -0.25, 4.0]), (n, 1)), np.tile(np.float32([0.75, -0.25, 4.5]), (n, 1))


def g_nonfinite(n, rng):
    """rigid pairs, a few of them with an inf or a NaN coordinate (what the dense path yields from zero-disparity taps)"""
    P, Q = g_rigid_out(n, rng)
    P, Q = P.astype(np.float32), Q.astype(np.float32)
    bad = np.arange(3, n, max(4, n // 6))
    for k, i in enumerate(bad):
        if k % 3 == 0:
            P[i, 2] = np.inf
        elif k % 3 == 1:
            Q[i, 0] = np.nan
        else:
            P[i] = [-np.inf, np.inf, np.inf]; Q[i, 2] = np.inf
    return P, Q


def g_rigid_sparse150(n, rng):
    """150 rigid pairs among outliers spread so widely that hardly any two of them are consistent"""
    A = _cloud(n, rng)
    Q = rng.uniform(-1000, 1000, (n, 3))
    sel = np.sort(rng.choice(n, 150, replace=False))
    Q[sel] = _move(A[sel], rng)
    return A, Q


def g_soft14(n, rng):
    """14 pairs, 4 of them displaced: the outlier pass leaves n2 = 10"""
    A = _cloud(n, rng)
    Q = _move(A, rng)
    Q[[1, 4, 8, 13]] += np.array([0.5, -0.5, 0.5])
    return A, Q


def g_all_nonfinite(n, rng):
    """no finite row at all: every count is 0, the seed row itself is non-finite"""
    A, Q = _cloud(n, rng).astype(np.float32), _cloud(n, rng).astype(np.float32)
    A[0::2, 0] = np.nan
    Q[1::2, 2] = np.inf
    return A, Q


GEOMETRY = dict(rigid_sparse150=g_rigid_sparse150, soft14=g_soft14, all_nonfinite=g_all_nonfinite,
                rigid=g_rigid, rigid_out=g_rigid_out, soft=g_soft, two_groups=g_two_groups, threshold=g_threshold, clique_one=g_clique_one,
                dup=g_dup, planar_frontal=g_planar_frontal, planar_tilted=g_planar_tilted, near_planar=g_near_planar, mirrored=g_mirrored,
                x8=g_x8, motion_1e6=g_motion_1e6, identical=g_identical, nonfinite=g_nonfinite)
# sets whose covariance has rank < 2 (compared through rc and, up to 1024 pairs, bit for bit with the restatement -- a Jacobi
# result on them means nothing) and sets with non-finite members (NaN transforms)
RANK_DEFICIENT = ("threshold", "clique_one", "identical")
SPECIAL = ("rigid_sparse150", "soft14", "all_nonfinite", "nonfinite")      # fixed sizes / non-finite members
ALL_BUILDERS = ("rigid_out", "two_groups", "threshold", "dup", "planar_frontal", "planar_tilted", "near_planar", "mirrored", "x8",
                "motion_1e6", "identical", "nonfinite")


def geometry(name, n, seed=0):
    rng = np.random.default_rng([seed, n, zlib.crc32(name.encode())])
    pa, pb = GEOMETRY[name](n, rng)
    return np.ascontiguousarray(pa, np.float32).reshape(-1, 3), np.ascontiguousarray(pb, np.float32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- the fit
def np_fit(src, dst):
    """-> (T 3x4 float64 or None, rc, s2/s1 of the covariance): rc 0 ok, -1 fewer than 3 points, -2 fewer than two non-zero
    singular values.  A non-finite input gives a NaN transform with rc 0, as a sum of its coordinates does."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    n = len(src)
    if n < 3:
        return None, -1, 0.0
    ms = (src.astype(np.longdouble).sum(0) / n).astype(np.float64)
    md = (dst.astype(np.longdouble).sum(0) / n).astype(np.float64)
    with np.errstate(invalid="ignore"):
        s, d = src.astype(np.float64) - ms, dst.astype(np.float64) - md
    with np.errstate(invalid="ignore"):
        cov = d.T @ s / n
    if not np.isfinite(cov).all():
        return np.full((3, 4), np.nan), 0, 1.0
    var = float((s * s).sum()) / n
    U, w, Vt = np.linalg.svd(cov)
    if np.count_nonzero(w) < 2:
        return None, -2, 0.0
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ np.diag(S) @ Vt
    scale = float(w @ S) / var
    T = np.empty((3, 4))
    T[:, :3] = R
    T[:, 3] = md - scale * (R @ ms)
    return T, 0, float(w[1] / w[0])


def residuals(T, pa, pb):
    """relative residual on homogeneous 4-vectors, float64"""
    a, b = pa.astype(np.float64), pb.astype(np.float64)
    r = b - (a @ T[:, :3].T + T[:, 3])
    return np.sqrt((r * r).sum(1)) / np.sqrt((b * b).sum(1) + 1.0)


def np_pose_fit(qa, qb, outlier_thr=OUTLIER, min_matches=MIN_MATCHES):
    """first fit + single-pass outlier rule (np.median) + final fit on the n1 pairs behind the clique filter
    -> dict(n2, rc1, rc2, T1, T2, nan, cond (the smaller s2/s1 of the fits made), gap (distance of the nearest residual to the
    threshold, inf when no outlier pass ran))"""
    n1 = len(qa)
    out = dict(n2=n1, rc1=1, rc2=1, T1=None, T2=None, nan=0, cond=1.0, gap=np.inf)
    fa, fb = qa, qb
    if outlier_thr > 0 and n1 >= 10:
        out["T1"], out["rc1"], c = np_fit(qa, qb)
        if out["rc1"] == 0:
            out["cond"] = min(out["cond"], c)
            e = residuals(out["T1"], qa, qb)
            if np.isnan(e).any():
                out["nan"] = 1
                keep = np.zeros(n1, bool)
            else:
                thr = outlier_thr + float(np.median(e))
                keep = e < thr
                out["gap"] = float(np.abs(e - thr).min())
            fa, fb = qa[keep], qb[keep]
            out["n2"] = int(keep.sum())
    if out["n2"] >= min_matches:
        out["T2"], out["rc2"], c = np_fit(fa, fb)
        if out["rc2"] == 0:
            out["cond"] = min(out["cond"], c)
    return out


def restated(qa, qb, outlier_thr=OUTLIER, min_matches=MIN_MATCHES):
    """pose_fit_ref on the same pairs (n1 <= 1024) -> dict(n2, rc1, rc2, T1, T2)"""
    n2, rc1, rc2, T2 = PF.pose_fit(qa, qb, outlier_thr, min_matches)
    T1 = None
    if outlier_thr > 0 and len(qa) >= 10 and rc1 == 0:
        T1 = PF.umeyama(qa, qb)[0]
    return dict(n2=n2, rc1=rc1, rc2=rc2, T1=T1, T2=T2)


# ---------------------------------------------------------------------------------------------- a whole case
class Case:
    """nq query keypoints of which M must match, the M pairs' 3-D points from GEOMETRY[geom]; rigidity / outlier 0 = that pass off"""

    def __init__(self, name, nq, M, geom="rigid_out", rigidity=RIGIDITY, outlier=OUTLIER, min_matches=MIN_MATCHES, seed=0, path=""):
        self.name, self.nq, self.M, self.geom, self.rigidity, self.outlier, self.min_matches, self.seed, self.path = \
            name, nq, M, geom, rigidity, outlier, min_matches, seed, path

    def build(self):
        rng = np.random.default_rng([self.seed, self.nq, self.M])
        self.dq, self.dt, q, t = descriptors(self.nq, self.M, rng)
        nt = len(self.dt)
        self.xy_a = rng.uniform(0, 64, (self.nq, 2)).astype(np.float32)
        self.xy_b = rng.uniform(0, 64, (nt, 2)).astype(np.float32)
        self.xyz_a = _cloud(self.nq, rng).astype(np.float32)
        self.xyz_b = _cloud(nt, rng).astype(np.float32)
        pa, pb = geometry(self.geom, self.M, self.seed)
        self.xyz_a[q], self.xyz_b[t] = pa, pb
        return self

    def model(self, oracle):
        """-> dict(q, t, pa, pb, counts (M, n1, n2, flags), rc (rc1, rc2), T1, T2, cond, gap, keep): what the fused step must return"""
        q, t = matches(self.dq, self.dt)
        assert len(q) == self.M, "the construction gave %d matches, the case asks for %d" % (len(q), self.M)
        pa, pb = self.xyz_a[q], self.xyz_b[t]
        keep = np.ones(len(q), bool)
        if self.rigidity > 0 and len(q) > 0:
            keep = oracle.rigid_clique(pa, pb, self.rigidity) > 0
        qa, qb = pa[keep], pb[keep]
        f = np_pose_fit(qa, qb, self.outlier, self.min_matches)
        return dict(q=q, t=t, pa=pa, pb=pb, qa=qa, qb=qb, keep=keep, counts=(len(q), len(qa), f["n2"], 2 * f["nan"]), rc=(f["rc1"], f["rc2"]),
                    T1=f["T1"], T2=f["T2"], cond=f["cond"], gap=f["gap"])
