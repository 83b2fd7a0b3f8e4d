"""What the pyramidal Lucas-Kanade tracker of include/vo355.h MEANS, in plain numpy float64 on whole images and real-valued
interpolation -- not the tap-by-tap, 14-bit-weight form the kernels (openvo_amd/csrc/klt.hip) and their restatement (tests/klt_ref.py)
share.  Nothing here is imported from either.  The kernels and the restatement are held to it by tests/test_gpu_klt_definitions.py and
tests/test_klt_def.py: the pyramid by equality, ONE Lucas-Kanade step under a bound derived below, the eigenvalue rule wherever that
bound decides it, whole tracks within a distance measured between this file and the restatement on the CPU.

Units.  Image samples are carried in 1 / 32 grey level and gradients in Scharr units (32 x the derivative: weights 3 + 10 + 3 = 16
on a central difference over 2 px), as the header does, so G = sum grad grad^T and b = sum (J - I) grad carry the same factor 32^2 and
delta = -G^-1 b is in pixels; the eigenvalue rule reads lambda_min(G) 2^-20 / win^2 in exactly these units.

The bound on a fixed-point sample.  The header's sample is (w00 t0 + w01 t1 + w10 t2 + w11 t3 + r) >> sh with integer weights that sum
to 2^14.  Write e_k = w_k / 2^14 - omega_k for the difference from the true bilinear weight omega_k.  Three weights are rounded to
nearest: |e_k| <= 2^-15.  The fourth is what is left: e_3 = -(e_0 + e_1 + e_2), |e_3| <= 1.5 2^-14.  The errors sum to zero, so
sum e_k t_k = sum e_k (t_k - m) for any m; with m the mid-range of the four taps |t_k - m| <= range / 2 and sum |e_k| <= 3 2^-14:
    |sum e_k t_k| <= range 1.5 2^-14.
The shift rounds to the nearest unit of the result: half a unit more.  The unit is 1 / 32 grey level for an image sample computed
from taps in grey levels (>> 9 of a 14-bit scale), i.e. 1 / 64 grey level = 0.5 in the units carried here, and 1 Scharr unit for a
gradient sample, i.e. 0.5.  So, in the units carried here,
    |I_fixed - I| <= 32 range_I 1.5 2^-14 + 0.5,        |D_fixed - D| <= range_D 1.5 2^-14 + 0.5.
The weights themselves are float64 products rounded before rint: 2^-52 relative, covered by the slack _SLOP on the factor.

The bound on a step.  With per-sample bounds eI, eJ, eDx, eDy the entries of G and b move by at most
    dG11 = sum (2 |Dx| eDx + eDx^2), dG12 = sum (|Dx| eDy + |Dy| eDx + eDx eDy), dG22 likewise,
    db1 = sum (|J - I| eDx + (eI + eJ) (|Dx| + eDx)), db2 likewise,
|dG| <= the Frobenius norm of the first, |db| the 2-norm of the second, and for (G + dG)(delta + d) = -(b + db):
    |d| <= |G^-1| (|db| + |dG| |delta|) / (1 - |G^-1| |dG|),      |G^-1| = 1 / lambda_min(G),
valid while the quotient |G^-1| |dG| is below 1; otherwise the point is UNDECIDABLE.  By Weyl's inequality lambda_min moves by at
most |dG|, which is what decides the eigenvalue rule.  The kernel's own float64 step (a handful of roundings at 2^-53) is covered by
_ARITH; the float32 rounding of a reported position is added where a position is compared."""
import numpy as np

ST_EIG, ST_OUT, ST_NONFINITE, ST_FB = 1, 2, 4, 8
MUTANTS = ("half", "sobel", "dy_is_dx", "step_sign", "a12_sign", "grad_from_b", "delta_x2", "pyr_121", "pyr_edge", "pyr_floor", "pyr_size",
           "eig_max", "eig_win", "lost_edge", "zero_outside", "osc_full", "fb_unsquared", "fb_from_forward")
_SLOP = 1.0 + 2.0 ** -30
_K = 1.5 * 2.0 ** -14 * _SLOP
_ARITH = 1e-9                       # px: the kernel's float64 step against exact arithmetic on its integers
_BIG = 2.0 ** 30


def f32_half_ulp(v):
    """half the spacing of float32 at |v| (the rounding of a reported coordinate)"""
    return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


class Definition:
    """mut: the name of ONE deliberately wrong reading (MUTANTS) or None.  The mutants exist to show that the checks can refuse."""

    def __init__(self, mut=None):
        assert mut is None or mut in MUTANTS
        self.mut = mut

    # ---- pyramid ---------------------------------------------------------------------------------------------------------------------
    def _pad2(self, I, axis):
        n = I.shape[axis]
        I = np.moveaxis(I, axis, 0)
        if self.mut == "pyr_edge":
            P = np.pad(I, [(2, 2)] + [(0, 0)] * (I.ndim - 1), mode="symmetric") if n >= 2 else np.concatenate([I] * 5)
        elif n >= 3:
            P = np.pad(I, [(2, 2)] + [(0, 0)] * (I.ndim - 1), mode="reflect")
        elif n == 2:                # reflect once, then clamp: -2 -> 2 -> 0, -1 -> 1, 2 -> 0, 3 -> -1 -> 0
            P = np.stack([I[0], I[1], I[0], I[1], I[0], I[0]])
        else:                       # every index lands on the only sample
            P = np.concatenate([I] * 5)
        return np.moveaxis(P, 0, axis)

    def pyr_down(self, img):
        I = np.asarray(img).astype(np.float64)
        k = np.array([0, 1, 2, 1, 0]) / 4.0 if self.mut == "pyr_121" else np.array([1, 4, 6, 4, 1]) / 16.0
        for axis in (0, 1):
            n = I.shape[axis]
            P = self._pad2(I, axis)
            I = sum(k[j] * np.take(P, np.arange(j, j + n), axis=axis) for j in range(5))
            keep = np.arange(0, n, 2)
            if self.mut == "pyr_size" and n > 1:
                keep = keep[:n // 2]
            I = np.take(I, keep, axis=axis)
        return np.floor(I) if self.mut == "pyr_floor" else np.floor(I + 0.5)

    def pyramid(self, img, levels):
        p = [np.asarray(img).astype(np.float64)]
        for _ in range(levels - 1):
            p.append(self.pyr_down(p[-1]))
        return p

    # ---- gradient images ---------------------------------------------------------------------------------------------------------------
    def gradients(self, lvl):
        """(Dx, Dy), each (h + 2, w + 2): the Scharr difference at the integer pixels -1 .. w, -1 .. h (index + 1).  Every read is
        clamped, so a difference at x >= w reads only column w - 1 on its x side and the rows of that column on its y side -- what it
        reads at x = w; likewise x <= -1, and the same per row: the gradient ANYWHERE is the gradient at the coordinates clamped to
        -1 .. w, -1 .. h.  Written separably: a central difference along one axis, smoothed 3 / 10 / 3 along the other."""
        P = np.pad(lvl, 2, mode="constant" if self.mut == "zero_outside" else "edge")
        s = (4.0, 8.0, 4.0) if self.mut == "sobel" else (3.0, 10.0, 3.0)
        cx = P[:, 2:] - P[:, :-2]                               # (h + 4, w + 2)
        Dx = s[0] * cx[:-2] + s[1] * cx[1:-1] + s[2] * cx[2:]
        cy = P[2:, :] - P[:-2, :]                               # (h + 2, w + 4)
        Dy = s[0] * cy[:, :-2] + s[1] * cy[:, 1:-1] + s[2] * cy[:, 2:]
        return Dx, (Dx if self.mut == "dy_is_dx" else Dy)

    # ---- samples -----------------------------------------------------------------------------------------------------------------------
    def sample(self, F, lo, cx, cy, win):
        """Real bilinear interpolation of F (whose index 0 is the coordinate `lo`, reads clamped to its extent) at
        c - (win - 1) / 2 + (u, v), u, v = 0 .. win - 1, for n positions -> (values, tap range), each (n, win, win)."""
        half = win / 2.0 if self.mut == "half" else (win - 1) / 2.0
        H, W = F.shape
        k = np.arange(win + 1)
        fr, idx, inside = [], [], []
        for c, n in ((np.asarray(cx, np.float64), W), (np.asarray(cy, np.float64), H)):
            t = c - half
            fl = np.floor(t)
            fr.append(t - fl)
            i = np.clip(fl, -_BIG, _BIG).astype(np.int64)[:, None] + k - lo
            inside.append((i >= 0) & (i < n))
            idx.append(np.clip(i, 0, n - 1))
        P = F[idx[1][:, :, None], idx[0][:, None, :]]
        if self.mut == "zero_outside":
            P = np.where(inside[1][:, :, None] & inside[0][:, None, :], P, 0.0)
        fx, fy = fr[0][:, None, None], fr[1][:, None, None]
        rows = (1.0 - fx) * P[:, :, :-1] + fx * P[:, :, 1:]
        val = (1.0 - fy) * rows[:, :-1, :] + fy * rows[:, 1:, :]
        taps = np.stack([P[:, :-1, :-1], P[:, :-1, 1:], P[:, 1:, :-1], P[:, 1:, 1:]])
        return val, taps.max(axis=0) - taps.min(axis=0)

    def template(self, A, gA, c, win):
        """I (1 / 32 grey level), Dx, Dy at c (n, 2) with their bounds, G, its bound and eigenvalues"""
        I, rI = self.sample(A, 0, c[:, 0], c[:, 1], win)
        Dx, rx = self.sample(gA[0], -1, c[:, 0], c[:, 1], win)
        Dy, ry = self.sample(gA[1], -1, c[:, 0], c[:, 1], win)
        T = dict(I=32.0 * I, eI=32.0 * rI * _K + 0.5, Dx=Dx, Dy=Dy, ex=rx * _K + 0.5, ey=ry * _K + 0.5)
        ax = (1, 2)
        T["G11"], T["G12"], T["G22"] = (Dx * Dx).sum(ax), (Dx * Dy).sum(ax), (Dy * Dy).sum(ax)
        d11 = (2 * np.abs(Dx) * T["ex"] + T["ex"] ** 2).sum(ax)
        d22 = (2 * np.abs(Dy) * T["ey"] + T["ey"] ** 2).sum(ax)
        d12 = (np.abs(Dx) * T["ey"] + np.abs(Dy) * T["ex"] + T["ex"] * T["ey"]).sum(ax)
        T["dG"] = np.sqrt(d11 * d11 + 2 * d12 * d12 + d22 * d22)
        tr, df = T["G11"] + T["G22"], T["G11"] - T["G22"]
        root = np.sqrt(df * df + 4.0 * T["G12"] * T["G12"])
        T["lmin"], T["lmax"] = 0.5 * (tr - root), 0.5 * (tr + root)
        T["D"] = T["G11"] * T["G22"] - T["G12"] * T["G12"]
        return T

    def eig_rule(self, T, win, min_eig):
        """-> (skip, decided): the level is skipped iff lambda_min(G) 2^-20 / win^2 < min_eig or D <= 0; decided only where the
        bound on G leaves no doubt (and G is not so ill-conditioned that the float64 determinant could change sign)"""
        lam = T["lmax"] if self.mut == "eig_max" else T["lmin"]
        s = 2.0 ** -20 / (win if self.mut == "eig_win" else win * win)
        skip = (lam * s < min_eig) | (T["D"] <= 0)
        sure_run = ((lam - T["dG"]) * s > min_eig) & (T["lmin"] - T["dG"] > 1e-9 * T["lmax"])
        sure_skip = (lam + T["dG"]) * s < min_eig
        return skip, np.where(skip, sure_skip, sure_run)

    def solve(self, T, J, eJ, sel=slice(None)):
        """delta = -G^-1 b for the image samples J (1 / 32 grey level) against the template rows `sel`, with its bound"""
        ax = (1, 2)
        Dx, Dy, ex, ey = T["Dx"][sel], T["Dy"][sel], T["ex"][sel], T["ey"][sel]
        dI = J - T["I"][sel]
        b1, b2 = (dI * Dx).sum(ax), (dI * Dy).sum(ax)
        G11, G12, G22, D = T["G11"][sel], T["G12"][sel], T["G22"][sel], T["D"][sel]
        o = -G12 if self.mut == "a12_sign" else G12
        with np.errstate(divide="ignore", invalid="ignore"):
            dx, dy = -(G22 * b1 - o * b2) / D, -(G11 * b2 - o * b1) / D
            if self.mut == "step_sign":
                dx, dy = -dx, -dy
            if self.mut == "delta_x2":
                dx, dy = 2 * dx, 2 * dy
            e = T["eI"][sel] + eJ
            db = np.hypot((np.abs(dI) * ex + e * (np.abs(Dx) + ex)).sum(ax), (np.abs(dI) * ey + e * (np.abs(Dy) + ey)).sum(ax))
            lmin, dG = T["lmin"][sel], T["dG"][sel]
            quot = np.where(lmin > 0, dG / lmin, np.inf)
            bound = np.where(quot < 1, (db + dG * np.hypot(dx, dy)) / (lmin * (1 - quot)), np.inf) + _ARITH
        return dx, dy, bound

    def step(self, A_L, B_L, c, q, win):
        """ONE Lucas-Kanade step of the window at c (n, 2) of level image A_L from the position q (n, 2) in B_L
        -> (delta (n, 2), bound (n,) on |delta_fixed - delta|, inf = undecidable)"""
        A_L, B_L = np.asarray(A_L, np.float64), np.asarray(B_L, np.float64)
        c, q = np.asarray(c, np.float64).reshape(-1, 2), np.asarray(q, np.float64).reshape(-1, 2)
        T = self.template(A_L, self.gradients(B_L if self.mut == "grad_from_b" else A_L), c, win)
        J, rJ = self.sample(B_L, 0, q[:, 0], q[:, 1], win)
        dx, dy, bound = self.solve(T, 32.0 * J, 32.0 * rJ * _K + 0.5)
        return np.stack([dx, dy], 1), bound

    # ---- the whole tracker ---------------------------------------------------------------------------------------------------------------
    def _one_way(self, pa, pb, ga, p0, win, iters, eps, min_eig, osc_step=None):
        """-> q (n, 2) at level 0, status, decided (the eigenvalue rule of every level visited was decided), margin (the smallest
        distance, in level-0 pixels, of any LOST test and of the final in-image test from its threshold)"""
        n, levels = len(p0), len(pa)
        h0, w0 = pa[0].shape
        q = p0 / 2.0 ** (levels - 1)
        status, dead = np.zeros(n, np.uint8), np.zeros(n, bool)
        decided, margin = np.ones(n, bool), np.full(n, np.inf)
        for L in range(levels - 1, -1, -1):
            hL, wL = pa[L].shape
            idx = np.nonzero(~dead)[0]
            if len(idx):
                T = self.template(pa[L], ga[L], p0[idx] / 2.0 ** L, win)
                skip, sure = self.eig_rule(T, win, min_eig)
                decided[idx] &= sure
                if L == 0:
                    status[idx[skip]] |= ST_EIG
                live = np.nonzero(~skip)[0]
                prev = np.zeros((len(idx), 2))
                r = 0.0 if self.mut == "lost_edge" else float(win)
                for k in range(iters):
                    if not len(live):
                        break
                    g = idx[live]
                    room = np.minimum(np.minimum(q[g, 0] + r, (wL - 1) + r - q[g, 0]), np.minimum(q[g, 1] + r, (hL - 1) + r - q[g, 1]))
                    margin[g] = np.minimum(margin[g], np.abs(room) * 2.0 ** L)
                    gone = g[~(room >= 0)]
                    status[gone] |= ST_OUT
                    dead[gone] = True
                    q[gone] *= 2.0 ** L
                    live = live[room >= 0]
                    g = idx[live]
                    if not len(live):
                        break
                    J, rJ = self.sample(pb[L], 0, q[g, 0], q[g, 1], win)
                    dx, dy, _ = self.solve(T, 32.0 * J, 32.0 * rJ * _K + 0.5, live)
                    q[g, 0] += dx
                    q[g, 1] += dy
                    small = dx * dx + dy * dy <= eps * eps
                    osc = ~small & (k >= 1) & (np.abs(dx + prev[live, 0]) < 0.01) & (np.abs(dy + prev[live, 1]) < 0.01)
                    back = 1.0 if self.mut == "osc_full" else 0.5
                    q[g[osc], 0] -= back * dx[osc]
                    q[g[osc], 1] -= back * dy[osc]
                    if osc_step is not None and L == 0:
                        osc_step[g[osc]] = np.hypot(dx[osc], dy[osc])
                    prev[live, 0], prev[live, 1] = dx, dy
                    live = live[~(small | osc)]
            if L > 0:
                q[~dead] *= 2.0
        alive = ~dead
        room = np.minimum(np.minimum(q[:, 0], (w0 - 1) - q[:, 0]), np.minimum(q[:, 1], (h0 - 1) - q[:, 1]))
        margin[alive] = np.minimum(margin[alive], np.abs(room[alive]))
        status[alive & ~(room >= 0)] |= ST_OUT
        return q, status, decided, margin

    def track_def(self, a, b, xy, win=21, levels=4, iters=30, eps=0.01, min_eig=1e-4, fb=1.0, pyr=None):
        """the tracker of the header on real samples -> dict: xy (n, 2) float32, status (n,), decided (n,: every eigenvalue rule on
        the way was decided), margin (n,: LOST and in-image tests, px), fb_margin (n,: |round trip - fb|, inf where none was made), round_trip (n,: its length,
        NaN where none was completed), osc_step (n,: the length of the step at which the forward pass ended LEVEL 0 by the oscillation
        stop, 0 where it did not)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        out, status = xy.copy(), np.zeros(n, np.uint8)
        decided, margin, fbm = np.ones(n, bool), np.full(n, np.inf), np.full(n, np.inf)
        res = dict(xy=out, status=status, decided=decided, margin=margin, fb_margin=fbm, round_trip=np.full(n, np.nan), osc_step=np.zeros(n))
        if n == 0:
            return res
        pa, pb = pyr if pyr is not None else (self.pyramid(a, levels), self.pyramid(b, levels))
        ga, gb = [self.gradients(l) for l in pa], [self.gradients(l) for l in pb]
        fin = np.isfinite(xy).all(axis=1)
        status[~fin] = ST_NONFINITE
        f = np.nonzero(fin)[0]
        if len(f):
            osc = np.zeros(len(f))
            q, st, dec, mg = self._one_way(pa, pb, gb if self.mut == "grad_from_b" else ga, xy[f].astype(np.float64), win, iters, eps, min_eig, osc)
            res["osc_step"][f] = osc
            out[f], status[f], decided[f], margin[f] = q.astype(np.float32), st, dec, mg
        g = np.nonzero(status == 0)[0]
        if fb > 0 and len(g):
            qb, stb, dec, mg = self._one_way(pb, pa, ga if self.mut == "grad_from_b" else gb, out[g].astype(np.float64), win, iters, eps, min_eig)
            back = qb.astype(np.float32).astype(np.float64)
            frm = out[g].astype(np.float64) if self.mut == "fb_from_forward" else xy[g].astype(np.float64)
            d = np.hypot(back[:, 0] - frm[:, 0], back[:, 1] - frm[:, 1])
            bad = (stb != 0) | ~((d * d <= fb) if self.mut == "fb_unsquared" else (d * d <= fb * fb))
            status[g[bad]] |= ST_FB
            decided[g] &= dec
            margin[g] = np.minimum(margin[g], mg)
            res["round_trip"][g] = np.where(stb == 0, d, np.nan)
            fbm[g] = np.where(stb == 0, np.abs(d - (np.sqrt(fb) if self.mut == "fb_unsquared" else fb)), np.inf)
        return res


# ---- holding a result to the definition ----------------------------------------------------------------------------------------------
def check_pyramid(levels_got, img, mut=None):
    """every level of a pyramid of img against the definition, by equality -> the number of differing pixels (0 = held); a level of
    another shape counts whole"""
    want = Definition(mut).pyramid(img, len(levels_got))
    bad = 0
    for g, w in zip(levels_got, want):
        g = np.asarray(g)
        bad += int((g.astype(np.float64) != w).sum()) if g.shape == w.shape else max(g.size, w.size)
    return bad


def check_step(a, b, xy, got, win, mut=None):
    """got = the (xy_out, status, iters) of a call with levels = 1, iters = 1, eps = 0, min_eig = 0, fb = 0 from finite starts xy inside
    +-win of the image: xy_out must be xy + delta within the derived bound plus the float32 rounding.  -> dict of figures;
    `violations` = decidable points outside their bound (0 = held)."""
    d = Definition(mut)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    p0 = xy.astype(np.float64)
    delta, bound = d.step(a, b, p0, p0, win)
    want = p0 + delta
    ok = np.isfinite(bound)
    tol = bound + np.hypot(f32_half_ulp(want[:, 0]), f32_half_ulp(want[:, 1]))
    with np.errstate(invalid="ignore"):
        err = np.hypot(got[0][:, 0].astype(np.float64) - want[:, 0], got[0][:, 1].astype(np.float64) - want[:, 1])
        ratio = np.where(ok, err / tol, 0.0)
    moved = ok & (got[2] == 1) & ((got[1] & ~np.uint8(ST_OUT)) == 0)       # a decidable point must have taken its one step
    viol = ok & (~moved | ~(ratio <= 1.0))
    return dict(n=len(xy), violations=int(viol.sum()), worst_ratio=float(ratio.max()) if len(xy) else 0.0, undecidable=float((~ok).mean()) if len(xy) else 0.0,
                median_bound=float(np.median(bound[ok])) if ok.any() else float("nan"),
                median_step=float(np.median(np.hypot(delta[ok, 0], delta[ok, 1]))) if ok.any() else float("nan"))


def check(a, b, xy, got, tau, mut=None, **prm):
    """got = (xy_out, status, iters) of a whole call with the parameters prm, held to track_def: a non-finite input comes back in its
    bits with status 4 and no iteration; wherever the definition decides the status (every eigenvalue rule decided by the bound on G,
    every LOST / in-image test further than tau from its threshold, the round trip further than 2 tau from fb) the status byte is the
    definition's and the position lies within tau + the float32 rounding of it.
    -> dict of figures: `compared` points, `beyond` (position further than tau), `status_diff`, `worst` distance, `nonfinite_bad`."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    R = Definition(mut).track_def(a, b, xy, **prm)
    gx, gs, gi = got
    fin = np.isfinite(xy).all(axis=1)
    nf_bad = int((~fin & ((gs != ST_NONFINITE) | (gi != 0) | (gx.view(np.uint32) != xy.view(np.uint32)).any(axis=1))).sum())
    dec = fin & R["decided"] & (R["margin"] > tau) & (R["fb_margin"] > 2 * tau)
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.hypot(gx[:, 0].astype(np.float64) - R["xy"][:, 0], gx[:, 1].astype(np.float64) - R["xy"][:, 1])
    lim = tau + np.hypot(f32_half_ulp(R["xy"][:, 0]), f32_half_ulp(R["xy"][:, 1]))
    beyond = dec & ~(dist <= lim)
    sdiff = dec & (gs != R["status"])
    tracked = dec & (R["status"] == 0)
    return dict(n=len(xy), compared=int(dec.sum()), tracked=int(tracked.sum()), beyond=int(beyond.sum()), beyond_tracked=int((beyond & tracked).sum()),
                status_diff=int(sdiff.sum()), worst=float(dist[dec & ~beyond].max()) if (dec & ~beyond).any() else 0.0,
                worst_all=float(np.nanmax(np.where(dec, dist, 0.0))) if dec.any() else 0.0, nonfinite_bad=nf_bad,
                dist=dist, decided=dec, status=R["status"], fb_margin=R["fb_margin"])
