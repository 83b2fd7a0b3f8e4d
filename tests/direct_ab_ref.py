"""numpy restatement of the dense direct alignment with the affine brightness term (include/vo355.h, vo_direct_align_ab): test
infrastructure, in the manner of tests/direct_ref.py, whose helpers it imports.

Everything through I_b is direct_ref.align's.  The state carries (k, m) from (1, 0) over iterations and levels, the residual is
(k I_b + m) - A, iterations it < `held` of a level take the six pose unknowns (29 sums), the others eight (46 sums: j[6] = I_b,
j[7] = 1), the solve is cholesky_solve below (any N, the operations in the order of csrc/pn_solve.h), and the pose, k and m are
committed together or not at all.  held = 2 is the header's definition; another value is a VARIANT, there only so that
tests/test_direct_ab_ref.py can print what the held iterations are for.

The decision margin is direct_ref.align's and additionally covers the distance of every new k from 0 (the k <= 0 decision).
sum_dtype=np.longdouble: the terms in float64 as ever, summed in extended precision (the referee)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_ref as DR                    # noqa: E402
import klt_ref as KR                       # noqa: E402
import pnp_refine_ref as PR                # noqa: E402

HELD = 2
NSUMS = {6: 29, 8: 46}


def cholesky_solve(H, g):
    """d with H d = -g for a symmetric N x N H, or None when a pivot is not positive: the operations of pn_solve<N> in their order
    (every product subtracted on its own, ascending k)."""
    n = len(g)
    L = np.zeros((n, n))
    for j in range(n):
        s = float(H[j, j])
        for k in range(j):
            s -= L[j, k] * L[j, k]
        if not s > 0.0:
            return None
        dj = math.sqrt(s)
        L[j, j] = dj
        for i in range(j + 1, n):
            v = float(H[i, j])
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / dj
    y = np.zeros(n)
    for i in range(n):
        v = -float(g[i])
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v / L[i, i]
    d = np.zeros(n)
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v -= L[k, i] * d[k]
        d[i] = v / L[i, i]
    return d


def full_information(sums, unknowns):
    """8 x 8 from the packed sums of a linearisation with 6 or 8 unknowns (zero outside the 6 x 6 block for 6)"""
    nh = unknowns * (unknowns + 1) // 2
    T = np.zeros((unknowns, unknowns))
    T[np.triu_indices(unknowns)] = np.asarray(sums[:nh], np.float64)
    F = np.zeros((8, 8))
    F[:unknowns, :unknowns] = T + np.triu(T, 1).T
    return F


def marginal(full, unknowns):
    """the 6 x 6 pose information marginalised over the brightness: H_pp - H_pb H_bb^-1 H_bp (the plain block for 6 unknowns)"""
    P = full[:6, :6].copy()
    if unknowns == 8:
        P = P - full[:6, 6:] @ np.linalg.solve(full[6:, 6:], full[6:, :6])
        P = 0.5 * (P + P.T)
    return P


def align(A, B, disp16, Q, K4, Rt0=None, roi=None, levels=3, iters=8, max_points=16384, grad_min=8, huber=10.0, dmin=4.0, dmax=100.0,
          z_min=0.1, min_pixels=64, sum_dtype=np.float64, held=HELD):
    """-> dict: the fields of Context.direct_align(affine=True)'s (status, iters_done, s, selected, n_first, n_last, wr2_first, wr2_last,
    Rt, gain, offset, unknowns, sums (44), information_full, information, g (8), count, wr2) + margin, n_huber, sums_abs (44, laid
    out like sums) and trace (per evaluated iteration: level, it, unknowns, participants, wr2, the pose and (k, m) it was evaluated at)."""
    A, B, disp16 = np.asarray(A, np.uint8), np.asarray(B, np.uint8), np.asarray(disp16, np.int16)
    h, w = A.shape
    assert B.shape == A.shape == disp16.shape and 1 <= levels <= DR.MAX_LEVELS and 3 <= iters <= 20
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(v) for v in K4)
    Rt = np.eye(4)[:3].copy() if Rt0 is None else np.array(Rt0, np.float64).reshape(-1, 4)[:3].copy()
    bk, bm = 1.0, 0.0
    pa, pb = KR.pyramid(A, levels), KR.pyramid(B, levels)
    rects = [DR.level_rect(pa[l].shape[1], pa[l].shape[0], w, h, roi, l) for l in range(levels)]
    out = dict(status=0, iters_done=0, s=np.array([DR.lattice_step(r, max_points) for r in rects], np.int32),
               selected=np.zeros(levels, np.int32), n_first=np.zeros(levels, np.int32), n_last=np.zeros(levels, np.int32),
               wr2_first=np.zeros(levels), wr2_last=np.zeros(levels), margin=np.inf, n_huber=0, trace=[])
    last, last_abs, last_nu = np.zeros(29), np.zeros(29), 6
    with np.errstate(all="ignore"):
        for l in range(levels - 1, -1, -1):
            x_lo, x_hi, y_lo, y_hi = rects[l]
            s, f = int(out["s"][l]), 1 << l
            Al, Bl = pa[l].astype(np.int64), pb[l].astype(np.float64)
            ys, xs = np.meshgrid(y_lo + 1 + s * np.arange(DR.lattice_n(y_lo, y_hi, s)), x_lo + 1 + s * np.arange(DR.lattice_n(x_lo, x_hi, s)),
                                 indexing="ij")
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
                nu = 6 if it < held else 8
                nh = nu * (nu + 1) // 2
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
                r = (bk * Ib + bm) - a_val[part]
                ar = np.abs(r)
                wt = np.where(ar <= huber, 1.0, huber / ar)
                gx_, gy_ = gfx[part], gfy[part]
                a0, a1, a2 = gx_ / zp, gy_ / zp, -((gx_ * xp + gy_ * yp) / (zp * zp))
                cols = [yp * a2 - zp * a1, zp * a0 - xp * a2, xp * a1 - yp * a0, a0, a1, a2]
                if nu == 8:
                    cols += [Ib, np.ones(len(r))]
                j = np.stack(cols)
                wj = wt * j
                tri = np.triu_indices(nu)
                terms = np.concatenate([wj[tri[0]] * j[tri[1]], wj * r, np.ones((1, len(r))), ((wt * r) * r)[None]])
                S = np.asarray(terms.astype(sum_dtype).sum(axis=1), np.float64)
                S_abs = np.abs(terms).sum(axis=1)
                n = int(S[nh + nu])
                out["n_huber"] += int((wt < 1.0).sum())
                out["trace"].append(dict(level=l, it=it, unknowns=nu, n=n, wr2=float(S[nh + nu + 1]), Rt=Rt.copy(), km=(bk, bm)))
                if it == 0:
                    out["n_first"][l], out["wr2_first"][l] = n, S[nh + nu + 1]
                out["n_last"][l], out["wr2_last"][l] = n, S[nh + nu + 1]
                if n < min_pixels:
                    out["status"] = 2
                    break
                dlt = None
                if np.isfinite(S).all():
                    Hm = np.zeros((nu, nu))
                    Hm[tri] = S[:nh]
                    dlt = cholesky_solve(Hm + np.triu(Hm, 1).T, S[nh:nh + nu])
                new = None
                nk, nm = bk, bm
                if dlt is not None:
                    E = PR.exp_so3(dlt[:3])
                    new = np.hstack([E @ Rt[:, :3], (E @ Rt[:, 3] + dlt[3:6])[:, None]])
                    if nu == 8:
                        nk, nm = bk + float(dlt[6]), bm + float(dlt[7])
                        if np.isfinite(nk):
                            out["margin"] = min(out["margin"], abs(nk))
                if new is None or not np.isfinite(new).all() or not (np.isfinite(nk) and np.isfinite(nm) and nk > 0.0):
                    out["status"] = -1
                    break
                Rt, bk, bm, last, last_abs, last_nu = new, nk, nm, S, S_abs, nu
                out["iters_done"] += 1
            if out["status"] != 0:
                break
    nh = last_nu * (last_nu + 1) // 2
    sums, sums_abs = np.zeros(44), np.zeros(44)
    sums[:nh + last_nu], sums_abs[:nh + last_nu] = last[:nh + last_nu], last_abs[:nh + last_nu]
    full = full_information(sums, last_nu)
    g = np.zeros(8)
    g[:last_nu] = sums[nh:nh + last_nu]
    out.update(Rt=Rt, gain=bk, offset=bm, unknowns=last_nu, sums=sums, sums_abs=sums_abs, information_full=full,
               information=marginal(full, last_nu), g=g, count=int(last[nh + last_nu]), wr2=float(last[nh + last_nu + 1]))
    return out
