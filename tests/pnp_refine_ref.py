"""numpy restatement of the stereo PnP step's inlier refinement (include/vo355.h, vo_pnp_pair): test infrastructure.

Gauss-Newton on a FIXED inlier set, float64 throughout: residual (fx X'/Z' + cx - u, fy Y'/Z' + cy - v) with X' = R X + t, the
21 + 6 sums of J^T J and J^T r with d X' / d (w, v) = [-[X']x | I] taken by a sequential loop over the inliers, a 6x6 Cholesky
solve, the update R <- Exp(w) R, t <- Exp(w) t + v; exactly `steps` steps, no early exit.  Status 0 ok, 1 not attempted (fewer
than 6 inliers or no step asked for), -1 when a pivot was not positive or a value was not finite."""
import math

import numpy as np


def exp_so3(w):
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-4:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + A * W + B * (np.outer(w, w) - th2 * np.eye(3))


def normal_sums(Rt, X, uv, K4, order, dtype=np.float64):
    """(H 6x6, g 6): the sums of one step over the points `order` lists, taken in that order.  dtype: the type every term is
    computed and accumulated in (np.longdouble: the high-precision run of the same sums); H and g come back in it."""
    dt = dtype
    fx, fy, cx, cy = (dt(float(v)) for v in K4)
    R = np.asarray(Rt, np.float64).astype(dt)
    H, g = np.zeros((6, 6), dt), np.zeros(6, dt)
    one = dt(1)
    for i in order:
        x, y, z = R[:, :3] @ X[i].astype(dt) + R[:, 3]
        iz = one / z
        r = ((fx * x * iz + cx) - dt(uv[i, 0]), (fy * y * iz + cy) - dt(uv[i, 1]))
        zero = dt(0)
        a = ((fx * iz, zero, -fx * x * iz * iz), (zero, fy * iz, -fy * y * iz * iz))
        for e in range(2):
            a0, a1, a2 = a[e]
            j = np.array([a2 * y - a1 * z, a0 * z - a2 * x, a1 * x - a0 * y, a0, a1, a2], dt)
            H += np.outer(j, j)
            g += j * r[e]
    return H, g


def cholesky_solve(H, g):
    """d with H d = -g, or None when a pivot is not positive."""
    L = np.zeros((6, 6))
    for j in range(6):
        s = H[j, j] - float(L[j, :j] @ L[j, :j])
        if not s > 0.0:
            return None
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    d = np.zeros(6)
    for i in range(5, -1, -1):
        d[i] = (y[i] - float(L[i + 1:, i] @ d[i + 1:])) / L[i, i]
    return d


def refine(Rt, X, uv, K4, mask, steps, order=None, dtype=np.float64):
    """-> (Rt 3x4 float64, status, steps run).  order: the inliers' indices in the order to sum them (default ascending).
    dtype: the type of the sums (normal_sums); they are rounded to float64 for the solve and the update."""
    Rt = np.array(Rt, np.float64).reshape(3, 4)
    X, uv = np.asarray(X, np.float32).reshape(-1, 3), np.asarray(uv, np.float32).reshape(-1, 2)
    inl = np.flatnonzero(np.asarray(mask)) if order is None else np.asarray(order)
    if steps <= 0 or len(inl) < 6:
        return Rt, 1, 0
    for k in range(steps):
        with np.errstate(all="ignore"):
            H, g = normal_sums(Rt, X, uv, K4, inl, dtype)
            H, g = np.asarray(H, np.float64), np.asarray(g, np.float64)
            d = cholesky_solve(H, g) if np.isfinite(H).all() and np.isfinite(g).all() else None
            if d is None:
                return Rt, -1, k
            E = exp_so3(d[:3])
            new = np.hstack([E @ Rt[:, :3], (E @ Rt[:, 3] + d[3:])[:, None]])
        if not np.isfinite(new).all():
            return Rt, -1, k
        Rt = new
    return Rt, 0, steps
