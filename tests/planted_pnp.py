"""Inputs and the model for the planted-slot tests of the fused PnP step (vo_pnp_pair: k_pnp_prep in csrc/geom.hip, k_pnp_hyp ->
k_pnp_score -> k_pnp_finish in csrc/ransac.hip).  No GPU in here; tests/planted.py supplies descriptors, matches, motion and cloud.

A case plants two sparse slots so that the step meets a chosen (nq, M), a chosen set of unusable matches (a non-finite 3-D point
in slot a), n_in inliers at chosen places, a pixel noise, iters / RANSAC seed / refine steps and the match flags:

    inlier    xy_b[t] = float32(projection of R X + t  +  noise * N(0, 1))     (R, t) = planted._motion(), K4 below
    outlier   xy_b[t] uniform over the 640 x 480 image

model(case, O) computes what the step must return, never assuming it from the construction: the matches (numpy brute force; the
window / mutual / loop restatements for the flagged cases) -> the finite filter in match order -> O.ransac_pnp -> the refit
restated in float64 (pnp_refine_ref.refine), the same with the inliers summed in thread-strided order (grouped by i % 256: the
order a thread of k_pnp_finish meets them in), and with np.longdouble sums -- the plain high-precision reference.

GROUPS is the matrix of tests/test_gpu_planted_pnp.py; tests/test_planted_pnp_ref.py asserts on the model alone that every case
reaches the regime its name promises."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted as P                        # noqa: E402
import pnp_refine_ref as PR                # noqa: E402
import sparse_loop_ref as SL               # noqa: E402
import window_match_ref as WM              # noqa: E402

K4 = (500.0, 500.0, 320.0, 240.0)
IMG_W, IMG_H = 640.0, 480.0
THR, SEED, ITERS = 1.5, 4321, 64
RATIO = P.RATIO
NONFINITE = (np.nan, np.inf, -np.inf)


def project(X, K4=K4):
    """float64 pixel of the points X (frame a) seen from frame b"""
    R, t = P._motion()
    Y = np.asarray(X, np.float64) @ R.T + t
    return np.stack([K4[0] * Y[:, 0] / Y[:, 2] + K4[2], K4[1] * Y[:, 1] / Y[:, 2] + K4[3]], 1)


def planted_Rt():
    R, t = P._motion()
    return np.hstack([R, t[:, None]])


def strided_order(mask, threads=256):
    """the inliers grouped by i % threads, ascending inside a group: thread 0's points, then thread 1's, ..."""
    inl = np.flatnonzero(np.asarray(mask))
    return inl[np.lexsort((inl, inl % threads))]


class PnpCase:
    """nq query keypoints, M planted matches; bad: the matches (positions in match order) whose 3-D point is non-finite, or "all";
    n_in inliers among the usable ones (None: 70 %), at the compacted positions `inliers` lists (None: drawn); scene: the seed of
    the construction; dup: that many further queries copy the descriptor of a train that is already matched (what the cross-check
    must remove); loop / window / cross / roi: the match flags and the ROI origin; collinear: the matched 3-D points lie on one line.
    K4: the intrinsics the scene is projected with and the model scores under (a subclass with another camera sets its own)."""
    K4 = K4

    def __init__(self, name, nq, M, bad=(), n_in=None, noise=0.0, iters=ITERS, seed=SEED, refine=0, scene=0, inliers=None, cross=False, loop=None,
                 window=None, roi=None, dup=0, collinear=False):
        self.name, self.nq, self.M, self.n_in, self.noise, self.iters, self.seed, self.refine, self.scene = name, nq, M, n_in, noise, iters, seed, refine, scene
        self.bad = np.arange(M) if isinstance(bad, str) else np.asarray(sorted(bad), np.int64)
        self.inliers, self.cross, self.loop, self.window, self.roi, self.dup = inliers, cross, loop, window, roi, dup
        self.collinear = collinear
        self.n = M - len(self.bad)                     # usable correspondences of the plain matches
        self._model = None

    @property
    def flagged(self):
        return self.cross or self.loop is not None or self.window is not None

    def build(self):
        if hasattr(self, "dq"):
            return self
        rng = np.random.default_rng([self.scene, self.nq, self.M])
        Mp = self.M - self.dup
        self.dq, self.dt, q, t = P.descriptors(self.nq, Mp, rng)
        nt = len(self.dt)
        if self.dup:                                    # further queries that copy a matched train, one more bit flipped than any partner
            free = np.setdiff1d(np.arange(self.nq), q)
            dq_extra = np.sort(rng.choice(free, self.dup, replace=False))
            src = rng.choice(Mp, self.dup, replace=False)
            for k, qi in zip(src, dq_extra):
                self.dq[qi] = self.dt[t[k]]
                for bit in rng.choice(256, 3, replace=False):
                    self.dq[qi, bit >> 3] ^= np.uint8(1 << (bit & 7))
            order = np.argsort(np.concatenate([q, dq_extra]), kind="stable")
            q, t = np.concatenate([q, dq_extra])[order].astype(np.int32), np.concatenate([t, t[src]])[order].astype(np.int32)
        self.q0, self.t0 = q, t
        self.xy_a = np.stack([rng.uniform(0, IMG_W, self.nq), rng.uniform(0, IMG_H, self.nq)], 1).astype(np.float32)
        self.xy_b = np.stack([rng.uniform(0, IMG_W, nt), rng.uniform(0, IMG_H, nt)], 1).astype(np.float32)
        self.xyz_a = P._cloud(self.nq, rng).astype(np.float32)
        self.xyz_b = P._cloud(nt, rng).astype(np.float32)
        if self.collinear:
            s = np.linspace(-1.0, 1.0, len(q))
            self.xyz_a[q] = np.stack([2 * s, s, 4 + s], 1).astype(np.float32)
        self.rd_a = rng.integers(0, 256, (self.nq, 32), dtype=np.uint8)
        self.rd_b = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        # the first occurrence of every train among the matches carries the geometry (a duplicate shares its partner's pixel)
        first = np.zeros(len(q), bool)
        first[np.unique(t, return_index=True)[1]] = True
        use = np.ones(len(q), bool)
        use[self.bad] = False
        pos = np.flatnonzero(use & first)               # match positions that may be inliers
        comp = np.cumsum(use) - 1                       # match position -> compacted position
        n_in = int(round(0.7 * len(pos))) if self.n_in is None else self.n_in
        if self.inliers is not None:
            want = np.asarray(self.inliers, np.int64)
            inl = pos[np.isin(comp[pos], want)]
            assert len(inl) == len(want) == n_in, "%s: the inlier places are not all usable" % self.name
        else:
            inl = np.sort(rng.choice(pos, n_in, replace=False))
        self.inl_pos = inl
        uv = project(self.xyz_a[q[inl]], self.K4) + self.noise * rng.normal(0, 1, (len(inl), 2))
        self.xy_b[t[inl]] = uv.astype(np.float32)
        if self.window is not None:                     # slot a sees every matched point where it is: most partners lie inside a window
            R0 = self.xyz_a[q].astype(np.float64)
            Ka = self.K4
            self.xy_a[q] = np.stack([Ka[0] * R0[:, 0] / R0[:, 2] + Ka[2], Ka[1] * R0[:, 1] / R0[:, 2] + Ka[3]], 1).astype(np.float32)
        if self.loop is not None:                       # right partners: nine in ten agree up to two bits, the rest are unrelated
            agree = rng.random(len(q)) < 0.9
            for k in np.flatnonzero(agree & first):
                self.rd_b[t[k]] = self.rd_a[q[k]]
                for bit in rng.choice(256, 2, replace=False):
                    self.rd_b[t[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
        for k, p in enumerate(self.bad):                # (after the projections: an unusable match is never an inlier)
            self.xyz_a[q[p], k % 3] = NONFINITE[(k // 3) % 3]
        return self

    # ------------------------------------------------------------------------------------------ the model
    def plain_matches(self):
        return P.matches(self.dq, self.dt, RATIO)

    def flagged_matches(self):
        if self.window is None and not self.cross:
            q, t = self.plain_matches()
        else:
            rx, ry = self.window if self.window is not None else (1e9, 1e9)     # (no window: every train is a candidate)
            if self.cross:
                idx, dist, mutual, _ = WM.window_knn2_mutual(self.dq, self.dt, self.xy_a, self.xy_b, rx, ry)
            else:
                (idx, dist), mutual = WM.window_knn2(self.dq, self.dt, self.xy_a, self.xy_b, rx, ry), None
            q, t = WM.ratio_filter(idx, dist, RATIO)
            if mutual is not None:
                keep = mutual[q] > 0
                q, t = q[keep], t[keep]
        if self.loop is not None:
            q, t = SL.loop_gate(dict(rdesc=self.rd_a), dict(rdesc=self.rd_b), q, t, self.loop)
        return np.asarray(q, np.int32), np.asarray(t, np.int32)

    def model(self, O):
        """-> dict(mq, mt (the M matches), M, n, q, t, X, uv (compacted), ok, best_iter, best_count, counts, Rt, mask,
        status, steps, Rt64, Rt_strided, Rt_ld (the refit three ways), err (float64 reprojection error under the winner))"""
        if self._model is not None:
            return self._model
        self.build()
        mq, mt = self.flagged_matches()
        Xa = self.xyz_a[mq]
        ok = np.isfinite(Xa).all(1)
        X, q, t = np.ascontiguousarray(Xa[ok]), mq[ok], mt[ok]
        org = np.float32([0, 0] if self.roi is None else self.roi[:2])
        uv = np.ascontiguousarray((self.xy_b[t] + org).astype(np.float32)).reshape(-1, 2)
        n, K4 = len(q), self.K4
        m = dict(mq=mq, mt=mt, M=len(mq), n=n, ok=ok, q=q, t=t, X=X, uv=uv)
        if n >= 4:
            r = O.ransac_pnp(X, uv, K4, self.iters, THR, self.seed)
            m.update(best_iter=r["best_iter"], best_count=r["best_count"], counts=r["counts"], Rt=np.array(r["Rt"]).reshape(3, 4), mask=r["mask"].copy())
        else:                                           # fewer than 4: no pose, no inlier (include/vo355.h)
            m.update(best_iter=0, best_count=0, counts=np.zeros(self.iters, np.int32), Rt=np.zeros((3, 4)), mask=np.zeros(n, np.uint8))
        if m["best_count"] > 0:
            Y = X.astype(np.float64) @ m["Rt"][:, :3].T + m["Rt"][:, 3]
            with np.errstate(all="ignore"):
                p = np.stack([K4[0] * Y[:, 0] / Y[:, 2] + K4[2], K4[1] * Y[:, 1] / Y[:, 2] + K4[3]], 1)
                m["err"] = np.where(Y[:, 2] > 0, np.sqrt(((p - uv.astype(np.float64)) ** 2).sum(1)), np.inf)
        else:
            m["err"] = np.full(n, np.inf)
        a = (m["Rt"], X, uv, K4, m["mask"], self.refine)
        m["Rt64"], m["status"], m["steps"] = PR.refine(*a)
        if m["status"] == 0:
            m["Rt_strided"], s2, k2 = PR.refine(*a, order=strided_order(m["mask"]))
            m["Rt_ld"], s3, k3 = PR.refine(*a, dtype=np.longdouble)
            assert (s2, k2, s3, k3) == (0, self.refine, 0, self.refine)
        else:
            m["Rt_strided"] = m["Rt_ld"] = m["Rt64"]
        self._model = m
        return m


# ---------------------------------------------------------------------------------------------- the matrix
def _bad_patterns(M):
    four = {257: (1, 100, 255, 256), 513: (1, 300, 511, 512), 1025: (1, 300, 600, 1024)}[M]       # (257 matches make two passes only)
    return [("match0", [0]), ("m255_m256", [255, 256]), ("wave1_of_pass0", range(64, 128)), ("pass0", range(256)),
            ("every_second", range(0, M, 2)), ("all_but_four", [i for i in range(M) if i not in four])]


def _prep():
    out = [PnpCase("nq%d_M%d" % (nq, M), nq, M) for nq, M in ((2, 2), (64, 64), (65, 65), (255, 255), (256, 256), (257, 257), (300, 257),
                                                             (513, 513), (1030, 1025), (4096, 40), (4096, 1025))]
    for M in (257, 513, 1025):
        out += [PnpCase("M%d_bad_%s" % (M, name), M + 5, M, bad=bad) for name, bad in _bad_patterns(M)]
    out.append(PnpCase("M600_all_unusable", 600, 600, bad="all"))
    return out


B_N = (4, 5, 63, 64, 65, 255, 256, 257, 1025)
B_ITERS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
B_PAIRS = sorted({(n, i) for n in B_N for i in (64, 257)} | {(65, i) for i in B_ITERS} | {(4, 1), (4, 1025), (1025, 1), (1025, 1025)})
# noise-free ties: 60 correspondences, 10 inliers, 1025 hypotheses; the scene seeds were found by the loop of
# test_planted_pnp_ref.py::test_the_tie_scenes_can_be_found_again, one first maximum per wave of k_pnp_finish
TIE_SCENES = dict(tie_first_pass=1, tie_late_wave0=4, tie_late_wave1=3, tie_late_wave2=9, tie_late_wave3=65)
# RANSAC seeds under which so few hypotheses still hold a good one, the LAST of them the winner (found by a loop over 1 .. 400)
FEW_ITERS_SEEDS = {(65, 1): 6, (65, 3): 6, (65, 4): 9, (65, 5): 23, (1025, 1): 1}


def _tie(name, scene):
    return PnpCase(name, 64, 60, n_in=10, noise=0.0, iters=1025, scene=scene)


def _score():
    out = [PnpCase("n%d_iters%d" % (n, i), n + 3, n, n_in=int(round(0.7 * n)), noise=1.0, iters=i, seed=FEW_ITERS_SEEDS.get((n, i), SEED)) for n, i in B_PAIRS]
    out += [_tie(name, scene) for name, scene in TIE_SCENES.items()]
    # every pixel random AND the 3-D points on one line: P3P has no pose for any sample, so no hypothesis reprojects even its own
    # three points (with points in general position every hypothesis scores at least those three)
    out.append(PnpCase("no_inlier_anywhere", 68, 65, n_in=0, collinear=True))
    return out


REFIT_SCENES = {1024: 1}          # (scene 0 leaves one of the 1024 planted inliers outside the winner's mask)


def _refit():
    out = []
    for c, total, steps in ((5, 12, (1, 5)), (6, 12, (1, 5, 20)), (7, 12, (1, 5)), (255, 320, (1, 5)), (256, 320, (1, 5)), (257, 320, (1, 5, 20)),
                            (513, 640, (1, 5)), (1024, 1280, (1, 5)), (2400, 3000, (1, 5))):
        out += [PnpCase("count%d_of_%d_refine%d" % (c, total, s), total + 3, total, n_in=c, noise=0.3, refine=s, scene=REFIT_SCENES.get(c, 0)) for s in steps]
    # the gate of the refit with noise-free inliers: the winner's mask is the planted set, 5 / 6 / 7 of 12
    out += [PnpCase("gate_noise_free_%d_of_12" % c, 15, 12, n_in=c, noise=0.0, refine=5) for c in (5, 6, 7)]
    out.append(PnpCase("inliers300_none_in_wave0", 603, 600, n_in=300, noise=0.3, refine=5,
                       inliers=[i for i in range(600) if i % 256 >= 64][:300]))
    out.append(PnpCase("inliers300_second_pass_on", 603, 600, n_in=300, noise=0.3, refine=5, inliers=range(256, 556)))
    return out


def _flags():
    kw = dict(n_in=400, noise=0.3, refine=3)
    return [PnpCase("cross_check_600_520", 600, 520, cross=True, dup=40, **kw),
            PnpCase("loop48_600_520", 600, 520, loop=48, **kw),
            PnpCase("window_600_520", 600, 520, window=(80, 60), **kw),
            PnpCase("all_flags_roi_600_520", 600, 520, cross=True, dup=40, loop=48, window=(80, 60), roi=(3, 5, 64, 64), **kw)]


GROUPS = dict(prep=_prep(), score=_score(), refit=_refit(), flags=_flags())
ALL_CASES = [(g, c.name) for g in GROUPS for c in GROUPS[g]]


def case(group, name):
    return next(c for c in GROUPS[group] if c.name == name)
