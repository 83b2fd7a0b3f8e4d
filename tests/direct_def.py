"""The sums of ONE linearisation of the dense direct alignment, written from the mathematics: test infrastructure (numpy + scipy).

tests/direct_ref.py transcribes the operation list of include/vo355.h, which csrc/direct.hip transcribes too: a wrong term in that list
-- a sign in the Jacobian, a mis-ordered twist -- would be in both.  This file shares none of those lines:

    the point        X = Q (x 2^l, y 2^l, d, 1)^T divided by its fourth component: the full 4 x 4 product
    the pose         T = [R t; 0 1], X' = T X; the update is the left-multiplied Exp(xi) T with xi = (omega, upsilon): rotations first
    the projection   pi(X') = K_l X' / z', K_l = K with all four entries divided by 2^l (level-l pixel coordinates are x / 2^l)
    the residual     r = I_b(pi(X')) - I_a(x), I_b bilinear (scipy.ndimage.map_coordinates, order 1), both images of pyramid level l
    the Jacobian     J_k = grad I_a(x) . dpi/dX' (2 x 3) . (G_k X')[:3], G_k the six 4 x 4 generators of se(3): the TEMPLATE's
                     gradient (np.gradient of the level image), evaluated once per point -- the inverse-compositional approximation
    the weight       Huber's: w = 1 for |r| <= k, k / |r| beyond; the cost rho(r) = r^2 / 2, or k (|r| - k / 2) beyond
    the sums         H = sum w J J^T, g = sum w J r, the count and sum w r^2, over the PARTICIPATING points: selected (on the lattice,
                     a disparity in [dmin, dmax], |grad I_a| >= grad_min), in front of z_min and projected where all four bilinear
                     taps lie inside the level's rectangle

The pyramid is klt_ref.pyramid (held to its own definition by the KLT suites)."""
import os
import sys

import numpy as np
from scipy.ndimage import map_coordinates

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                       # noqa: E402


def generators():
    """G_0..2 the rotations about x, y, z, G_3..5 the translations along them"""
    G = np.zeros((6, 4, 4))
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        G[k, b, a], G[k, a, b] = 1.0, -1.0
        G[3 + k, k, 3] = 1.0
    return G


GEN = generators()


def rectangle(shape_l, shape, roi, l):
    """[x_lo, x_hi) x [y_lo, y_hi) of level l: the level image, or the ROI (clipped to the image) divided by 2^l -- rounded up at its
    low edges and down at its high edges, so that the rectangle never leaves the ROI"""
    (h_l, w_l), (h, w) = shape_l, shape
    if roi is None:
        return 0, w_l, 0, h_l
    f = 2 ** l
    x0, y0, x1, y1 = (min(v, m) for v, m in zip(roi, (w, h, w, h)))
    return int(np.ceil(x0 / f)), int(np.floor(x1 / f)), int(np.ceil(y0 / f)), int(np.floor(y1 / f))


def lattice(rect, max_points):
    """the interior pixels of the rectangle on the coarsest-needed lattice: the smallest step s with at most max_points of them"""
    x_lo, x_hi, y_lo, y_hi = rect
    s = 1
    while True:
        xs, ys = range(x_lo + 1, x_hi - 1, s), range(y_lo + 1, y_hi - 1, s)
        if len(xs) * len(ys) <= max_points:
            return [(x, y) for y in ys for x in xs], s
        s += 1


def project(K_l, T, X):
    Xc = T @ X
    return np.array([K_l[0, 0] * Xc[0] / Xc[2] + K_l[0, 2], K_l[1, 1] * Xc[1] / Xc[2] + K_l[1, 2]]), Xc


def geometric_jacobian(K_l, Xc):
    """d pi(Exp(xi) X') / d xi at xi = 0 (2 x 6): dpi/dX' . [G_k X']"""
    x, y, z = Xc[:3]
    dpi = np.array([[K_l[0, 0] / z, 0.0, -K_l[0, 0] * x / z ** 2], [0.0, K_l[1, 1] / z, -K_l[1, 1] * y / z ** 2]])
    return dpi @ np.stack([(G @ Xc)[:3] for G in GEN], axis=1)


def huber_rho(r, k):
    a = np.abs(r)
    return np.where(a <= k, 0.5 * r * r, k * (a - 0.5 * k))


def linearise(A, B, disp16, Q, K4, Rt, level, roi=None, levels=3, max_points=16384, grad_min=8, huber=10.0, dmin=4.0, dmax=100.0, z_min=0.1,
              **_):
    """-> dict(H 6x6, g 6, count, wr2, s, selected, at: {(x, y): (r, w, J)} of the participating points)"""
    A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
    Ia, Ib = (KR.pyramid(I, levels)[level].astype(np.float64) for I in (A, B))
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    T = np.vstack([np.asarray(Rt, np.float64).reshape(-1, 4)[:3], [0, 0, 0, 1.0]])
    f = 2 ** level
    fx, fy, cx, cy = K4
    K_l = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, f]], np.float64) / f
    gy, gx = np.gradient(Ia)
    rect = rectangle(Ia.shape, A.shape, roi, level)
    x_lo, x_hi, y_lo, y_hi = rect
    pts, s = lattice(rect, max_points)
    H, g, count, wr2, selected, at = np.zeros((6, 6)), np.zeros(6), 0, 0.0, 0, {}
    for x, y in pts:
        d = disp16[y * f, x * f] / 16.0
        grad = np.array([gx[y, x], gy[y, x]])
        if not (dmin <= d <= dmax) or grad @ grad < grad_min ** 2:
            continue
        selected += 1
        X = Q @ np.array([x * f, y * f, d, 1.0])
        with np.errstate(all="ignore"):
            X = X / X[3]
            (u, v), Xc = project(K_l, T, X)
        if not (Xc[2] > z_min and x_lo <= u < x_hi - 1 and y_lo <= v < y_hi - 1):
            continue
        r = float(map_coordinates(Ib, [[v], [u]], order=1)[0]) - Ia[y, x]
        w = 1.0 if abs(r) <= huber else huber / abs(r)
        J = grad @ geometric_jacobian(K_l, Xc)
        H += w * np.outer(J, J)
        g += w * J * r
        wr2 += w * r * r
        count += 1
        at[(x, y)] = (r, w, J)
    return dict(H=H, g=g, count=count, wr2=wr2, s=s, selected=selected, at=at)
