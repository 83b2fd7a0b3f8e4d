"""numpy restatement of the dense direct alignment (include/vo355.h, vo_direct_align): test infrastructure.

float64 throughout, vectorised over the lattice, every product and sum of a term in the order the header writes it; only the sums
over the points are numpy's (pairwise) instead of the kernel's (per thread, wave tree, wave order), so the float64 results agree with
the kernel to rounding while every integer field -- status, iterations, s, the counts -- agrees exactly, PROVIDED no decision sits on
its bound: align() therefore also returns the smallest DECISION MARGIN, over all selected points and iterations the distance of z'
from z_min and, for the points in front of z_min, of u and v from the bounds they are tested against.

sum_dtype=np.longdouble: the terms are formed in float64 as ever and summed in extended precision (the referee when a float64
comparison exceeds its bar)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                       # noqa: E402
import pnp_refine_ref as PR                # noqa: E402

MAX_LEVELS = 4
TRIU = np.triu_indices(6)                  # packed upper triangle in row order


def lattice_n(lo, hi, s):
    return (hi - lo - 2 + s - 1) // s if hi - lo - 2 > 0 else 0


def level_rect(w_l, h_l, w, h, roi, l):
    """[x_lo, x_hi) x [y_lo, y_hi) of level l: the level image, or the ROI (clipped to the w x h image) scaled by ceiling at the low
    edges and floor at the high edges"""
    if roi is None:
        return 0, w_l, 0, h_l
    f = 1 << l
    x0, y0, x1, y1 = min(roi[0], w), min(roi[1], h), min(roi[2], w), min(roi[3], h)
    return -(-x0 // f), max(x1, 0) // f, -(-y0 // f), max(y1, 0) // f


def lattice_step(rect, max_points):
    s = 1
    while lattice_n(rect[0], rect[1], s) * lattice_n(rect[2], rect[3], s) > max_points:
        s += 1
    return s


def information(sums):
    H = np.zeros((6, 6))
    H[TRIU] = np.asarray(sums[:21], np.float64)
    return H + np.triu(H, 1).T


def align(A, B, disp16, Q, K4, Rt0=None, roi=None, levels=3, iters=8, max_points=16384, grad_min=8, huber=10.0, dmin=4.0, dmax=100.0,
          z_min=0.1, min_pixels=64, sum_dtype=np.float64):
    """-> dict: the fields of Context.direct_align's (status, iters_done, s, selected, n_first, n_last, wr2_first, wr2_last, Rt, sums,
    information, g, count, wr2) + margin (the smallest decision margin; inf when no point was ever tested), n_huber (terms with a
    weight below 1, over all iterations), sums_abs (per sum of `sums` the sum of its terms' magnitudes: the scale a summation
    error is measured against) and trace (per evaluated iteration: level, participants, wr2, the pose it was evaluated at)."""
    A, B, disp16 = np.asarray(A, np.uint8), np.asarray(B, np.uint8), np.asarray(disp16, np.int16)
    h, w = A.shape
    assert B.shape == A.shape == disp16.shape and 1 <= levels <= MAX_LEVELS and 1 <= iters <= 20
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(v) for v in K4)
    Rt = np.eye(4)[:3].copy() if Rt0 is None else np.array(Rt0, np.float64).reshape(-1, 4)[:3].copy()
    pa, pb = KR.pyramid(A, levels), KR.pyramid(B, levels)
    rects = [level_rect(pa[l].shape[1], pa[l].shape[0], w, h, roi, l) for l in range(levels)]
    out = dict(status=0, iters_done=0, s=np.array([lattice_step(r, max_points) for r in rects], np.int32),
               selected=np.zeros(levels, np.int32), n_first=np.zeros(levels, np.int32), n_last=np.zeros(levels, np.int32),
               wr2_first=np.zeros(levels), wr2_last=np.zeros(levels), margin=np.inf, n_huber=0, trace=[])
    last, last_abs = np.zeros(29), np.zeros(29)
    with np.errstate(all="ignore"):
        for l in range(levels - 1, -1, -1):
            x_lo, x_hi, y_lo, y_hi = rects[l]
            s, f = int(out["s"][l]), 1 << l
            Al, Bl = pa[l].astype(np.int64), pb[l].astype(np.float64)
            ys, xs = np.meshgrid(y_lo + 1 + s * np.arange(lattice_n(y_lo, y_hi, s)), x_lo + 1 + s * np.arange(lattice_n(x_lo, x_hi, s)), indexing="ij")
            xs, ys = xs.ravel(), ys.ravel()                  # linear index j nx + i
            d16 = disp16[ys * f, xs * f].astype(np.int64)
            gx2, gy2 = Al[ys, xs + 1] - Al[ys, xs - 1], Al[ys + 1, xs] - Al[ys - 1, xs]
            keep = (d16.astype(np.float64) >= 16.0 * dmin) & (d16.astype(np.float64) <= 16.0 * dmax) & (gx2 * gx2 + gy2 * gy2 >= 4 * grad_min * grad_min)
            xs, ys, d16, gx2, gy2 = xs[keep], ys[keep], d16[keep], gx2[keep], gy2[keep]
            out["selected"][l] = len(xs)
            a_val = Al[ys, xs].astype(np.float64)
            d = d16.astype(np.float64) / 16.0
            W = Q[3, 2] * d + Q[3, 3]
            X, Y, Z = ((xs * f).astype(np.float64) + Q[0, 3]) / W, ((ys * f).astype(np.float64) + Q[1, 3]) / W, Q[2, 3] / W
            fxl, fyl, cxl, cyl = fx / f, fy / f, cx / f, cy / f
            gfx, gfy = (0.5 * gx2.astype(np.float64)) * fxl, (0.5 * gy2.astype(np.float64)) * fyl
            for it in range(iters):
                R = Rt.ravel()
                xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[3]
                yc = ((R[4] * X + R[5] * Y) + R[6] * Z) + R[7]
                zc = ((R[8] * X + R[9] * Y) + R[10] * Z) + R[11]
                front = zc > z_min
                u, v = (fxl * xc) / zc + cxl, (fyl * yc) / zc + cyl
                part = front & (u >= x_lo) & (u < x_hi - 1) & (v >= y_lo) & (v < y_hi - 1)
                if len(xs):
                    m = [np.abs(zc - z_min).min()]
                    if front.any():
                        m += [np.abs(b_ - c_[front]).min() for c_, b_ in ((u, x_lo), (u, x_hi - 1), (v, y_lo), (v, y_hi - 1))]
                    m = np.array(m)
                    out["margin"] = min(out["margin"], float(m[np.isfinite(m)].min()) if np.isfinite(m).any() else 0.0)
                    if not np.isfinite(zc).all() or not np.isfinite(u[front]).all() or not np.isfinite(v[front]).all():
                        out["margin"] = 0.0            # (a non-finite coordinate has no margin: such a case is not comparable)
                u, v, xp, yp, zp = u[part], v[part], xc[part], yc[part], zc[part]
                fu, fv = np.floor(u), np.floor(v)
                ax, ay, iu, iv = u - fu, v - fv, fu.astype(np.int64), fv.astype(np.int64)
                Ib = (Bl[iv, iu] * (1.0 - ax) + Bl[iv, iu + 1] * ax) * (1.0 - ay) + (Bl[iv + 1, iu] * (1.0 - ax) + Bl[iv + 1, iu + 1] * ax) * ay
                r = Ib - a_val[part]
                ar = np.abs(r)
                wt = np.where(ar <= huber, 1.0, huber / ar)
                gx_, gy_ = gfx[part], gfy[part]
                a0, a1, a2 = gx_ / zp, gy_ / zp, -((gx_ * xp + gy_ * yp) / (zp * zp))
                j = np.stack([yp * a2 - zp * a1, zp * a0 - xp * a2, xp * a1 - yp * a0, a0, a1, a2])
                wj = wt * j
                terms = np.concatenate([wj[TRIU[0]] * j[TRIU[1]], wj * r, np.ones((1, len(r))), ((wt * r) * r)[None]])
                S = np.asarray(terms.astype(sum_dtype).sum(axis=1), np.float64)
                S_abs = np.abs(terms).sum(axis=1)
                n = int(S[27])
                out["n_huber"] += int((wt < 1.0).sum())
                out["trace"].append(dict(level=l, n=n, wr2=float(S[28]), Rt=Rt.copy()))
                if it == 0:
                    out["n_first"][l], out["wr2_first"][l] = n, S[28]
                out["n_last"][l], out["wr2_last"][l] = n, S[28]
                if n < min_pixels:
                    out["status"] = 2
                    break
                dlt = PR.cholesky_solve(information(S), S[21:27]) if np.isfinite(S).all() else None
                new = None
                if dlt is not None:
                    E = PR.exp_so3(dlt[:3])
                    new = np.hstack([E @ Rt[:, :3], (E @ Rt[:, 3] + dlt[3:])[:, None]])
                if new is None or not np.isfinite(new).all():
                    out["status"] = -1
                    break
                Rt, last, last_abs = new, S, S_abs
                out["iters_done"] += 1
            if out["status"] != 0:
                break
    out.update(Rt=Rt, sums=last[:27].copy(), information=information(last), g=last[21:27].copy(), count=int(last[27]), wr2=float(last[28]),
               sums_abs=last_abs[:27].copy())
    return out
