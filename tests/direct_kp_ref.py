"""numpy restatement of the patch alignment (include/vo355.h, vo_direct_align_kp): test infrastructure.

The points are the patch pixels of the keypoints that carry depth; everything from x' on is vo_direct_align's and is written here as
tests/direct_ref.py writes it: float64 throughout, every product and sum of a term in the header's order, only the sums over the points
are numpy's (pairwise) instead of the kernel's, so the float64 results agree with the kernel to rounding while every integer field
-- status, iterations, the keypoints in use, the counts -- agrees exactly, PROVIDED no decision sits on its bound.  align() therefore
returns the smallest DECISION MARGIN: direct_ref's (z' from z_min, u and v from their bounds, over all selected points and iterations)
and, for every usable keypoint and level, the distance of vx / 2^l and vy / 2^l from a rounding tie (a value k + 1 / 2).

sum_dtype=np.longdouble: the terms are formed in float64 as ever and summed in extended precision."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                       # noqa: E402
import pnp_refine_ref as PR                # noqa: E402
import direct_ref as DR                    # noqa: E402

TRIU = DR.TRIU


def usable(xy, xyz, w, h, origin=(0, 0)):
    """-> (vx, vy float64, Z float64, ok): the float32 addition of the crop origin, and the tests made BEFORE any integer is formed"""
    xy, xyz = np.asarray(xy, np.float32).reshape(-1, 2), np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        vx = (xy[:, 0] + np.float32(origin[0])).astype(np.float64)
        vy = (xy[:, 1] + np.float32(origin[1])).astype(np.float64)
        Z = xyz[:, 2].astype(np.float64)
        ok = np.isfinite(vx) & np.isfinite(vy) & np.isfinite(Z) & (Z > 0) & (vx >= 0) & (vx < w) & (vy >= 0) & (vy < h)
    return vx, vy, Z, ok


def level_points(vx, vy, ok, rect, l, patch):
    """-> (kp index, x, y) of every point of level l in ascending point index, the number of keypoints in use, the tie margin"""
    x_lo, x_hi, y_lo, y_hi = rect
    hp, f = patch // 2, float(1 << l)
    idx = np.flatnonzero(ok)
    fx_, fy_ = vx[idx] / f, vy[idx] / f
    tie = np.inf
    if len(idx):
        tie = float(min(np.abs(fx_ - np.floor(fx_) - 0.5).min(), np.abs(fy_ - np.floor(fy_) - 0.5).min()))
    cx, cy = np.rint(fx_).astype(np.int64), np.rint(fy_).astype(np.int64)          # half to even
    use = (cx - hp >= x_lo + 1) & (cx + hp <= x_hi - 2) & (cy - hp >= y_lo + 1) & (cy + hp <= y_hi - 2)
    idx, cx, cy = idx[use], cx[use], cy[use]
    dy, dx = np.meshgrid(np.arange(-hp, hp + 1), np.arange(-hp, hp + 1), indexing="ij")      # (dy + hp) patch + (dx + hp)
    dx, dy = dx.ravel(), dy.ravel()
    ki = np.repeat(idx, patch * patch)
    xs = (cx[:, None] + dx[None, :]).ravel()
    ys = (cy[:, None] + dy[None, :]).ravel()
    return ki, xs, ys, int(len(idx)), tie


def align(A, B, xy, xyz, Q, K4, Rt0=None, roi=None, levels=3, iters=4, patch=5, grad_min=8, huber=10.0, z_min=0.1, min_pixels=64,
          sum_dtype=np.float64):
    """xy: (n, 2) float32 keypoints in pixels of the ROI crop, xyz: (n, 3) float32 (its Z is read).  -> dict: the fields of
    Context.direct_align_kp's (status, iters_done, keypoints, selected, n_first, n_last, wr2_first, wr2_last, Rt, sums, information, g,
    count, wr2, patch) + margin, n_huber, sums_abs and trace as direct_ref.align returns them, + points (per level: the (kp, x, y) of
    the selected points; None for a level the step never reached) and in_use (per level: the indices of the keypoints in use)."""
    A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
    h, w = A.shape
    assert B.shape == A.shape and 1 <= levels <= DR.MAX_LEVELS and 1 <= iters <= 20 and patch in (3, 5, 7)
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    assert np.isfinite(Q[2, 3]) and Q[2, 3] != 0
    fx, fy, cx, cy = (float(v) for v in K4)
    Rt = np.eye(4)[:3].copy() if Rt0 is None else np.array(Rt0, np.float64).reshape(-1, 4)[:3].copy()
    pa, pb = KR.pyramid(A, levels), KR.pyramid(B, levels)
    rects = [DR.level_rect(pa[l].shape[1], pa[l].shape[0], w, h, roi, l) for l in range(levels)]
    vx, vy, Zk, ok = usable(xy, xyz, w, h, (0, 0) if roi is None else (roi[0], roi[1]))
    sk = Zk / Q[2, 3]
    out = dict(status=0, iters_done=0, keypoints=np.zeros(levels, np.int32), patch=patch,
               selected=np.zeros(levels, np.int32), n_first=np.zeros(levels, np.int32), n_last=np.zeros(levels, np.int32),
               wr2_first=np.zeros(levels), wr2_last=np.zeros(levels), margin=np.inf, n_huber=0, trace=[], points=[None] * levels, in_use=[None] * levels)
    last, last_abs = np.zeros(29), np.zeros(29)
    with np.errstate(all="ignore"):
        for l in range(levels - 1, -1, -1):
            x_lo, x_hi, y_lo, y_hi = rects[l]
            f = 1 << l
            Al, Bl = pa[l].astype(np.int64), pb[l].astype(np.float64)
            ki, xs, ys, n_use, tie = level_points(vx, vy, ok, rects[l], l, patch)
            out["keypoints"][l] = n_use
            out["in_use"][l] = np.unique(ki)
            out["margin"] = min(out["margin"], tie)
            gx2, gy2 = Al[ys, xs + 1] - Al[ys, xs - 1], Al[ys + 1, xs] - Al[ys - 1, xs]
            keep = gx2 * gx2 + gy2 * gy2 >= 4 * grad_min * grad_min
            ki, xs, ys, gx2, gy2 = ki[keep], xs[keep], ys[keep], gx2[keep], gy2[keep]
            out["selected"][l] = len(xs)
            out["points"][l] = (ki, xs, ys)
            a_val = Al[ys, xs].astype(np.float64)
            X, Y, Z = ((xs * f).astype(np.float64) + Q[0, 3]) * sk[ki], ((ys * f).astype(np.float64) + Q[1, 3]) * sk[ki], Zk[ki]
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
                dlt = PR.cholesky_solve(DR.information(S), S[21:27]) if np.isfinite(S).all() else None
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
    out.update(Rt=Rt, sums=last[:27].copy(), information=DR.information(last), g=last[21:27].copy(), count=int(last[27]), wr2=float(last[28]),
               sums_abs=last_abs[:27].copy())
    return out
