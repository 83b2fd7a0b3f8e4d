"""What an inlier IS, in float64, and which points a float32 evaluation can be held to.  numpy only: no GPU, no oracle.

The scoring kernels of csrc/ransac.hip (k_ransac_score / k_ransac_mask / k_mono_finish / k_mono_pose_finish through sampson_inlier,
k_pnp_score / k_pnp_mask / k_pnp_finish through reproj_inlier) and their restatements in oracle/src/ransac.c and pnp.c evaluate the
two tests below in float32.  This module states the tests themselves and bounds the float32 evaluation from outside:

    sampson(E, K4, p1, p2, thr)    F = K^-T E K^-1, x = (u, v, 1):
                                   d2 = (x2^T F x1)^2 / ((F x1)_0^2 + (F x1)_1^2 + (F^T x2)_0^2 + (F^T x2)_1^2)
                                   inlier iff d2 < float32(thr)^2
    reproj(Rt, K4, X, uv, thr)     Y = R X + t, inlier iff Y_z > 0 and |pi(Y) - uv|^2 < float32(thr)^2; evaluated in the
                                   division-free form of the kernel, |P X - uv z|^2 < thr^2 z^2 with P = K [R | t], z = (P X)_2

Both return a Decision: value (d2, or the squared reprojection error; inf behind the camera), inlier (the definition, float64),
sure_in and sure_out.  sure_in[i]: EVERY float32 evaluation that follows the kernel's operation order calls point i an inlier;
sure_out[i]: every one calls it an outlier.  A point with neither is undecidable: the definition's value is closer to the threshold
than float32 can resolve, and either answer is right.  A NaN coordinate makes the point sure_out (every comparison is `<` or `>`:
NaN gives false).

The bound.  u = 2^-24 is the unit roundoff of float32; U = u (1 + 2^-20) is used for it, the excess absorbing the second-order
terms ((1 + u)^k - 1 <= k U for k <= 5) and the rounding of this module's own float64 arithmetic.  A sum of products evaluated
left to right carries |computed - exact| <= k U sum|terms| where k counts the roundings the FIRST term passes through (every
other term passes through no more).  Fused multiply-adds only remove roundings, so the bound covers a contracted build too.
ETA = 2^-149 per operation covers a product that underflows.

  sampson_inlier, in its operation order:
    fx0 = (F0 u1 + F1 v1) + F2      F0 is a float32 ROUNDING of the float64 entry (1), times u1 (2), plus (3), plus (4):  K_IN = 4
                                    (fx1, fx2, ft0, ft1 alike)
    num = (u2 fx0 + v2 fx1) + fx2   fx0 carries its own error e0; times u2 (1), plus (2), plus (3):                      K_OUT = 3
                                    |num^ - num| <= |u2| e0 + |v2| e1 + e2 + 3 U (|u2|(|fx0| + e0) + |v2|(|fx1| + e1) + |fx2| + e2)
    den = ((fx0^2 + fx1^2) + ft0^2) + ft1^2     each square over the interval [|v| - e, |v| + e], rounded (1), three sums (4)
    d = (num num) / den             the square over its interval, rounded (1); the quotient bounded from both sides, rounded (1)
    thr2 = thr thr                  rounded (1):   sure_in  iff  d_hi < thr^2 (1 - U),   sure_out  iff  d_lo > thr^2 (1 + U)
  F is scaled to max |entry| = 1 as rs_emit scales it (the decision does not depend on the scale; the magnitudes of the bound do).
  The kernel builds F in float64 from the E it returns, this module builds it again: two 3-term products of |K^-1|^T |E| |K^-1|
  = A, entries of K^-1 with two roundings, the scaling -- at most 16 float64 roundings each way, so the two F differ by at most
  dF = 32 2^-53 A / max|F| entry by entry, carried through every form beside the float32 rounding.

  reproj_inlier:
    xc = ((P0 X + P1 Y) + P2 Z) + P3   P0 a float32 rounding (1), times X (2), three sums (5):                            K_PNP = 5
                                       (yc, zc alike; the float64 P of the kernel and of this module differ by at most
                                       dP = 4 2^-53 (|fx R| + |cx R_2|))
    du = xc - u zc                     a = e_xc + |u| e_zc + U |u| (|zc| + e_zc)  [the product], then the difference rounds:
                                       |du^ - du| <= a + U (|du| + a)
    e = du du + dv dv                  squares over their intervals, rounded (1), summed (2)
    lim = thr2 (zc zc)                 thr2 rounded (1), the square over its interval, rounded (2), the product (3)
    sure_in  iff  zc - e_zc > 0 and e_hi < lim_lo;    sure_out  iff  zc + e_zc <= 0 or e_lo > lim_hi

WRONG_SAMPSON / WRONG_REPROJ hold the mistakes a restatement would share with the kernel, as plain numpy definitions;
tests/test_score_ref.py shows that each of them moves DECIDABLE points of the scenes the GPU tests use."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24 * (1.0 + 2.0 ** -20)
ETA = 2.0 ** -149
K_IN, K_OUT, K_PNP = 4, 3, 5

Decision = namedtuple("Decision", "value inlier sure_in sure_out")


def thr2_of(thr):
    """float32(thr)^2 as a float64: the threshold of both definitions"""
    t = float(np.float32(thr))
    return t * t


def fundamental(E, K4):
    """-> (F = K^-T E K^-1 scaled to max |entry| 1, dF: the most the kernel's float64 F differs from it, entry by entry)"""
    fx, fy, cx, cy = (float(v) for v in K4)
    Ki = np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    E = np.asarray(E, np.float64).reshape(3, 3)
    F = Ki.T @ E @ Ki
    A = np.abs(Ki).T @ np.abs(E) @ np.abs(Ki)
    mx = float(np.abs(F).max())
    if not mx > 0.0:                                   # (no model: all-zero F, every point an outlier)
        return np.zeros((3, 3)), np.zeros((3, 3))
    return F / mx, 32.0 * 2.0 ** -53 * A / mx


def _pixels(p):
    return np.asarray(p, np.float32).reshape(-1, 2).astype(np.float64)


def _form3(c, dc, a, b):
    """c0 a + c1 b + c2 and the bound of its float32 evaluation with float32-rounded c"""
    v = c[0] * a + c[1] * b + c[2]
    s = np.abs(c[0] * a) + np.abs(c[1] * b) + abs(c[2])
    e = K_IN * U * s + (1.0 + 8.0 * U) * (dc[0] * np.abs(a) + dc[1] * np.abs(b) + dc[2]) + 3.0 * ETA
    return v, e


def _sq_interval(v, e):
    """[lo, hi] of x^2 over x in [v - e, v + e]"""
    a = np.abs(v)
    return np.maximum(a - e, 0.0) ** 2, (a + e) ** 2


def sampson(E, K4, p1, p2, thr):
    F, dF = fundamental(E, K4)
    p1, p2 = _pixels(p1), _pixels(p2)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    t2 = thr2_of(thr)
    with np.errstate(all="ignore"):
        fx0, e0 = _form3(F[0], dF[0], u1, v1)
        fx1, e1 = _form3(F[1], dF[1], u1, v1)
        fx2, e2 = _form3(F[2], dF[2], u1, v1)
        ft0, g0 = _form3(F[:, 0], dF[:, 0], u2, v2)
        ft1, g1 = _form3(F[:, 1], dF[:, 1], u2, v2)
        num = u2 * fx0 + v2 * fx1 + fx2
        au, av = np.abs(u2), np.abs(v2)
        e_num = (au * e0 + av * e1 + e2) + K_OUT * U * (au * (np.abs(fx0) + e0) + av * (np.abs(fx1) + e1) + (np.abs(fx2) + e2)) + 3.0 * ETA
        den = fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1
        lo = hi = 0.0
        for v, e in ((fx0, e0), (fx1, e1), (ft0, g0), (ft1, g1)):
            a, b = _sq_interval(v, e)
            lo, hi = lo + a, hi + b
        den_lo, den_hi = np.maximum(lo * (1.0 - 4.0 * U) - 4.0 * ETA, 0.0), hi * (1.0 + 4.0 * U) + 4.0 * ETA
        nn_lo, nn_hi = _sq_interval(num, e_num)
        nn_lo, nn_hi = np.maximum(nn_lo * (1.0 - U) - ETA, 0.0), nn_hi * (1.0 + U) + ETA
        d_lo = np.maximum(nn_lo / den_hi * (1.0 - U) - ETA, 0.0)
        d_hi = np.where(den_lo > 0.0, nn_hi / den_lo * (1.0 + U) + ETA, np.inf)
        value = num * num / den
        inlier = value < t2
        sure_in = d_hi < t2 * (1.0 - U)
        sure_out = d_lo > t2 * (1.0 + U)
    nan = np.isnan(p1).any(1) | np.isnan(p2).any(1)
    if not F.any():                                    # no model: every product is 0, 0 / 0 is never below the threshold
        nan = np.ones(len(p1), bool)
    return Decision(value, inlier & ~nan, sure_in & ~nan, sure_out | nan)


def projection(Rt, K4):
    """-> (P = K [R | t] 3x4, dP: the most the kernel's float64 P differs from it)"""
    fx, fy, cx, cy = (float(v) for v in K4)
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    P = np.stack([fx * Rt[0] + cx * Rt[2], fy * Rt[1] + cy * Rt[2], Rt[2]])
    dP = 4.0 * 2.0 ** -53 * np.stack([np.abs(fx * Rt[0]) + np.abs(cx * Rt[2]), np.abs(fy * Rt[1]) + np.abs(cy * Rt[2]), np.zeros(4)])
    return P, dP


def _form4(c, dc, X):
    v = c[0] * X[:, 0] + c[1] * X[:, 1] + c[2] * X[:, 2] + c[3]
    aX = np.abs(X)
    s = np.abs(c[0]) * aX[:, 0] + np.abs(c[1]) * aX[:, 1] + np.abs(c[2]) * aX[:, 2] + abs(c[3])
    e = K_PNP * U * s + (1.0 + 8.0 * U) * (dc[0] * aX[:, 0] + dc[1] * aX[:, 1] + dc[2] * aX[:, 2] + dc[3]) + 4.0 * ETA
    return v, e


def reproj(Rt, K4, X, uv, thr):
    P, dP = projection(Rt, K4)
    X = np.asarray(X, np.float32).reshape(-1, 3).astype(np.float64)
    uv = _pixels(uv)
    t2 = thr2_of(thr)
    with np.errstate(all="ignore"):
        xc, ex = _form4(P[0], dP[0], X)
        yc, ey = _form4(P[1], dP[1], X)
        zc, ez = _form4(P[2], dP[2], X)
        lo = hi = err = 0.0
        for c, e, w in ((xc, ex, uv[:, 0]), (yc, ey, uv[:, 1])):
            d = c - w * zc
            a = e + np.abs(w) * ez + U * np.abs(w) * (np.abs(zc) + ez) + ETA
            ed = a + U * (np.abs(d) + a)
            s_lo, s_hi = _sq_interval(d, ed)
            lo, hi, err = lo + s_lo, hi + s_hi, err + d * d
        e_lo, e_hi = np.maximum(lo * (1.0 - 2.0 * U) - 3.0 * ETA, 0.0), hi * (1.0 + 2.0 * U) + 3.0 * ETA
        z_lo, z_hi = _sq_interval(zc, ez)
        lim_lo, lim_hi = np.maximum(t2 * z_lo * (1.0 - 3.0 * U) - 2.0 * ETA, 0.0), t2 * z_hi * (1.0 + 3.0 * U) + 2.0 * ETA
        inlier = (zc > 0.0) & (err < t2 * zc * zc)
        value = np.where(zc > 0.0, err / (zc * zc), np.inf)
        sure_in = (zc - ez > 0.0) & (e_hi < lim_lo)
        sure_out = (zc + ez <= 0.0) | (e_lo > lim_hi)
    nan = np.isnan(X).any(1) | np.isnan(uv).any(1)
    if not P.any():                                    # no model: zc is exactly 0, never in front of the camera
        nan = np.ones(len(X), bool)
    return Decision(value, inlier & ~nan, sure_in & ~nan, sure_out | nan)


def undecidable(d):
    return ~(d.sure_in | d.sure_out)


def disagreements(d, mask):
    """the decidable points on which a mask contradicts the definition"""
    mask = np.asarray(mask).astype(bool)
    return np.flatnonzero((d.sure_in & ~mask) | (d.sure_out & mask))


# ---- the mistakes --------------------------------------------------------------------------------------------------------------
def _sampson_terms(E, K4, p1, p2):
    F, _ = fundamental(E, K4)
    p1, p2 = _pixels(p1), _pixels(p2)
    h1, h2 = np.c_[p1, np.ones(len(p1))], np.c_[p2, np.ones(len(p2))]
    Fx, Ftx = h1 @ F.T, h2 @ F
    return (h2 * Fx).sum(1), Fx, Ftx


def wrong_epipolar_image2(E, K4, p1, p2, thr):
    """distance to the epipolar line in image 2 alone -- which IS Sampson's distance without its two F^T x2 terms"""
    num, Fx, _ = _sampson_terms(E, K4, p1, p2)
    with np.errstate(all="ignore"):
        return num * num / (Fx[:, 0] ** 2 + Fx[:, 1] ** 2) < thr2_of(thr)


def wrong_epipolar_image1(E, K4, p1, p2, thr):
    """the same mistake the other way round: without the two F x1 terms"""
    num, _, Ftx = _sampson_terms(E, K4, p1, p2)
    with np.errstate(all="ignore"):
        return num * num / (Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2) < thr2_of(thr)


def wrong_threshold_not_squared(E, K4, p1, p2, thr):
    return sampson(E, K4, p1, p2, thr).value < float(np.float32(thr))


def wrong_transposed_E(E, K4, p1, p2, thr):
    return sampson(np.asarray(E, np.float64).reshape(3, 3).T, K4, p1, p2, thr).inlier


def wrong_no_depth_rule(Rt, K4, X, uv, thr):
    P, _ = projection(Rt, K4)
    Y = np.c_[np.asarray(X, np.float32).reshape(-1, 3).astype(np.float64), np.ones(len(X))] @ P.T
    w = _pixels(uv)
    return (Y[:, 0] - w[:, 0] * Y[:, 2]) ** 2 + (Y[:, 1] - w[:, 1] * Y[:, 2]) ** 2 < thr2_of(thr) * Y[:, 2] ** 2


def wrong_focals_swapped(Rt, K4, X, uv, thr):
    return reproj(Rt, (K4[1], K4[0], K4[2], K4[3]), X, uv, thr).inlier


# name -> (function, applies(K4, thr, scene has points behind the camera))
WRONG_SAMPSON = {
    "epipolar_image2": (wrong_epipolar_image2, lambda K4, thr: True),
    "epipolar_image1": (wrong_epipolar_image1, lambda K4, thr: True),
    "threshold_not_squared": (wrong_threshold_not_squared, lambda K4, thr: float(np.float32(thr)) != 1.0),
    "transposed_E": (wrong_transposed_E, lambda K4, thr: True),
}
WRONG_REPROJ = {
    "no_depth_rule": (wrong_no_depth_rule, lambda K4, thr, behind: behind),
    "focals_swapped": (wrong_focals_swapped, lambda K4, thr, behind: K4[0] != K4[1]),
}
