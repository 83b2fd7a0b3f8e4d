"""Inputs of the sweep-group tests: stereo pairs whose post filters have work to do, and the conditions that say so.

pair(w, h, k, D, minD) is pair number k of a shape: smoothed noise, the right image the left one shifted by a background
disparity that differs from pair to pair, with small foreground blobs at a nearer disparity copied into it.  A blob is 8 x 10
pixels: below any speckle window the tests use, more than speckleRange away from its background -- the speckle filter removes
it -- and it occludes what lies beside it, which the left-right check removes.

Coverage.get(...) computes the oracle's disparity of such a pair and measures, on the oracle alone, what the filters did to
it; the asserts in there make a silent loss of coverage a failure."""
import weakref

import numpy as np


def params(D=64, speckle=150, minD=0, **over):
    p = dict(minDisparity=minD, numDisparities=D, blockSize=5, P1=200, P2=800, disp12MaxDiff=1, preFilterCap=63,
             uniquenessRatio=10, speckleWindowSize=speckle, speckleRange=2)
    p.update(over)
    return p


def pair(w, h, k, D=64, minD=0):
    rng = np.random.default_rng([w, h, k])
    pad = 16 + D + abs(minD)
    base = rng.integers(0, 256, (h, w + 2 * pad), dtype=np.uint8).astype(np.int32)
    sm = base.copy()
    sm[:, 1:] += base[:, :-1]
    sm[:, 0] += base[:, 0]
    sm[1:, :] += base[:-1, :]
    sm[0, :] += base[0, :]
    base = (sm // 3).astype(np.uint8)
    lo, hi = minD + 1, minD + D - 2
    d_bg = lo + (3 * k + 1) % max(1, hi - lo - 9)
    d_fg = d_bg + 5 + k % 3
    L = base[:, pad:pad + w].copy()
    R = base[:, pad + d_bg:pad + d_bg + w].copy()
    x_first = max(minD + D, 0) + 4
    for row_index, y0 in enumerate(range(2 + k % 3, h - 8, 19)):
        for x0 in range(x_first + (7 * row_index + 3 * k) % 11, w - 10, 37):
            if x0 - d_fg < 0 or x0 - d_fg + 10 > w:
                continue
            R[y0:y0 + 8, x0 - d_fg:x0 - d_fg + 10] = L[y0:y0 + 8, x0:x0 + 10]
    return L, R


def band(w, p):
    """(minX1, W1): the columns SGBM computes"""
    minD, D = p["minDisparity"], p["numDisparities"]
    x0 = max(minD + D, 0)
    return x0, w + min(minD, 0) - x0


def standard(p):
    """the parameter set the coverage conditions are stated under, at the disparity range of p and with its speckle filter on
    or off: a case that turns one parameter to an extreme (a window above the image size invalidates every pixel, whatever
    the input) shows on the same pair under this set that its input gives the filters work"""
    return params(p["numDisparities"], 150 if p["speckleWindowSize"] > 0 else 0, p["minDisparity"])


def valid_share(d16, w, p):
    x0, W1 = band(w, p)
    return float((d16[:, x0:x0 + W1] >= p["minDisparity"] * 16).mean())


class Coverage:
    """oracle disparity of pair k of a shape under parameters p, and what the post filters removed from that pair -- computed
    once per (shape, parameters, pair) and never changed afterwards.

    Every member: at least 80 % of the computed band is valid.  Shapes with W1 >= 48 and 17 rows or more, speckle filter on:
    it changes at least 20 pixels of every member.  Every group: the left-right check and the speckle filter each remove at
    least one pixel, and no two members have the same disparity.  These are measured on the oracle under standard(p); no two
    members' disparities under p itself are alike either, unless p leaves no pixel valid at all.
    fuzz=True (parameters drawn at random): half of the band is valid in the disparity the test compares, and no two members
    of a group are alike in it."""

    def __init__(self, oracle):
        self.oracle, self.memo = oracle, {}

    def entry(self, w, h, k, p, mode=0, fuzz=False):
        """the record of a pair, nothing asserted (`share`: valid share of the band, of `ref` for a fuzz draw)"""
        key = (w, h, k, mode, fuzz) + tuple(sorted(p.items()))
        if key not in self.memo:
            L, R = pair(w, h, k, p["numDisparities"], p["minDisparity"])
            run = self.oracle.sgbm_compute
            ref = run(L, R, p, mode)
            q, std, speckle_px, lr_px = p, ref, None, None
            if not fuzz:
                q = standard(p)
                std = ref if (q == p and mode == 0) else run(L, R, q, 0)
                lr_px = int((std != run(L, R, dict(q, disp12MaxDiff=1000), 0)).sum())
                if q["speckleWindowSize"] > 0:
                    speckle_px = int((std != run(L, R, dict(q, speckleWindowSize=0), 0)).sum())
            for a in (L, R, ref, std):
                a.setflags(write=False)
            self.memo[key] = dict(L=L, R=R, ref=ref, std=std, speckle_px=speckle_px, lr_px=lr_px, share=valid_share(std, w, q),
                                  any_valid=bool((ref >= p["minDisparity"] * 16).any()))
        return self.memo[key]

    def get(self, w, h, k, p, mode=0, fuzz=False):
        c = self.entry(w, h, k, p, mode, fuzz)
        assert c["share"] >= (0.5 if fuzz else 0.8), ("valid share of the computed band", w, h, k, p, c["share"])
        if c["speckle_px"] is not None and band(w, p)[1] >= 48 and h >= 17:
            assert c["speckle_px"] >= 20, ("pixels the speckle filter changes", w, h, k, p, c["speckle_px"])
        return c

    def group(self, w, h, ks, p, mode=0, fuzz=False):
        """the members of one group -- pairs ks of a shape -- with the conditions that hold per group"""
        m = [self.get(w, h, k, p, mode, fuzz) for k in ks]
        for i in range(len(m)):
            for j in range(i):
                assert not np.array_equal(m[i]["std"], m[j]["std"]), ("two members with one disparity", w, h, ks[i], ks[j])
                if m[i]["any_valid"] or m[j]["any_valid"]:
                    assert not np.array_equal(m[i]["ref"], m[j]["ref"]), ("two members with one disparity", w, h, p, ks[i], ks[j])
        if not fuzz:
            assert sum(c["lr_px"] for c in m) >= 1, ("pixels the left-right check removes", w, h, ks, p)
            if p["speckleWindowSize"] > 0:
                assert sum(c["speckle_px"] for c in m) >= 1, ("pixels the speckle filter changes", w, h, ks, p)
        return m


def disp16(ctx, slot, w, h):
    return np.rint(ctx.download_disparity_f32(slot, (h, w)) * 16).astype(np.int16)


def check(ctx, want, slot, w, h, what):
    """the slot's disparity against want = (oracle, the pair swept alone), bit for bit, all three ways"""
    ref, alone = want
    got = disp16(ctx, slot, w, h)
    assert np.array_equal(alone, ref), (what, "alone vs oracle", int((alone != ref).sum()))
    assert np.array_equal(got, ref), (what, "group vs oracle", int((got != ref).sum()))
    assert np.array_equal(got, alone), (what, "group vs alone")


class Refs:
    """the two references of a pair: the oracle's disparity (with the coverage conditions of Coverage) and the disparity of the
    same pair streamed with group size 1 through the context under test -- once per context, shape, parameters and pair.  The
    run at group size 1 uses a slot of its own, away from the ones the groups under test fill."""

    def __init__(self, oracle, slot=27):
        self.cov, self.slot, self.alone = Coverage(oracle), slot, weakref.WeakKeyDictionary()

    def get(self, ctx, w, h, k, p, mode=0, fuzz=False):
        c = self.cov.get(w, h, k, p, mode, fuzz)
        memo = self.alone.setdefault(ctx, {})
        key = (w, h, k, mode) + tuple(sorted(p.items()))
        if key not in memo:
            ctx.set_sgbm(p, mode)
            assert ctx.set_sweep_group(1) == 1
            ctx.prefetch_pair(self.slot, c["L"], c["R"], True)
            assert ctx.sweep_group_stats()["open"] == 0                # group size 1 never defers
            memo[key] = disp16(ctx, self.slot, w, h)
            memo[key].setflags(write=False)
        return c["ref"], memo[key]

    def group(self, ctx, w, h, ks, p, mode=0, fuzz=False):
        self.cov.group(w, h, ks, p, mode, fuzz)
        return [self.get(ctx, w, h, k, p, mode, fuzz) for k in ks]
