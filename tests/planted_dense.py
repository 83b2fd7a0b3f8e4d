"""Inputs and plain references for the planted-DENSE-slot tests: the bilinear depth lookup of the default path (bilinear_one over
TapDisp with reproject_px under it, csrc/geom.hip) in k_points3d, the second loop of k_pose_prep and of k_pnp_prep, and the
per-pixel part alone in k_reproject_disp16 / k_disp_to_f32.  No GPU in here; tests/planted.py and tests/planted_pnp.py supply
descriptors, matches and the models of the two fused steps.

The definition (oracle/src/geom.c):
    pixel    homg = Q [x y d 1]^T summed left to right in float64, d = float32(disp16) / 16;  out_i = float32(homg_i), then
             out_i = float32(float64(out_i) * (1 / homg_3))               -- W == 0 gives +-inf (or NaN where homg_i == 0)
    lookup   taps (fx, fy), (fx, fy + 1), (fx + 1, fy), (fx + 1, fy + 1) of the CROPPED image, in that order;  a tap is used iff it
             exists in the crop and none of its coordinates is +-inf (NaN and the finite negative invalid value ARE used);  weights in
             float64, rounded to float32 for the float32 product and the float32 running sum `num`;  `den` summed in float64,
             rounded to float32 for the float32 division.  status 0 | 1 (a NaN in the result) | 2 (no tap used: NaN triple)

    lookup(disp16, Q, roi, xy)      the numpy restatement in that operation order -> (xyz (n, 3) float32, status (n,) uint8)
    exact(disp16, Q, roi, xy)       the same definition with np.longdouble throughout (no float32 rounding anywhere)
    classify(disp16, Q, roi, xy)    the regime every keypoint hits: hole taps, existing taps, status, edge kind, mixed signs, ...
    FIELDS / QS / ROIS / positions  the inputs;  DenseCase / DensePnpCase the cases of the two fused steps

CPU figures (tests/test_planted_dense_ref.py prints them; properties of the inputs and of the restatement, not GPU results):
    restatement against np.longdouble      largest deviation 2.45 float32 ulps over every field x Q x ROI x position set, on keypoints
                                           whose used taps do not mix signs in a coordinate (asserted below ULP_BOUND = 8: two roundings
                                           per pixel, two per product, three sums, the rounding of den and the division -- nine
                                           half-ulps and no cancellation -- rounded up to the next power of two)
    pose cases (M, n1, n2, flags)          all valid (60, 60, 60, 0) and (280, 280, 280, 0); renormalised (60, 60, 60, 0) with 20 renormalised
                                           matches; status 1, filter on | off (60, 41, 41, 0) | (60, 60, 0, 2); status 2 (60, 49, 49, 1); both,
                                           filter off (280, 280, 0, 3); last column (60, 59, 59, 0); Q[3,3] != 0 with both (60, 34, 34, 1)
    PnP cases (M, n, flags)                (200, 200, 0), (200, 143, 1), (300, 214, 1), wave 1 unusable (300, 236, 1), pass 0 unusable
                                           (300, 44, 1), (40, 3, 1), cross-check 300 -> 270 matches, 193 usable
"""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted as P                        # noqa: E402
import planted_pnp as PP                   # noqa: E402

W, H = 96, 64
INVALID16 = (0 - 1) * 16                   # (minDisparity - 1) * 16 with minDisparity 0: what SGBM writes into an invalid pixel
ULP_BOUND = 8.0


def _q_plain():
    Q = np.eye(4)
    Q[3, 3] = 0.0; Q[2, 3] = 50.0; Q[3, 2] = 10.0
    return Q


# plain: the planted suites' Q (W = 10 d: zero disparity is the hole).  w33: Q[3,3] != 0, W = 8 d - 4 == 0 exactly at d16 = 8 -- a
# hole at a NON-zero disparity, while zero disparity gives a finite point (W = -4)
QS = dict(plain=_q_plain(), w33=np.array([[1.0, 0, 0, -48.0], [0, 1.0, 0, -32.0], [0, 0, 0, 50.0], [0, 0, 8.0, -4.0]]))
HOLE16 = dict(plain=0, w33=8)              # the disparity value that is a hole under each Q
# the camera each Q describes, as the PnP step takes it (x_img = fx X / Z + cx)
K4S = dict(plain=(50.0, 50.0, 0.0, 0.0), w33=(50.0, 50.0, 48.0, 32.0))
ROIS = dict(none=None, inner=(3, 5, 80, 50), clipped=(3, 5, 200, 100))


def crop(roi, w, h):
    """-> (x0, y0, x1, y1) of the crop: numpy slice semantics, the far edge clipped by the image"""
    if roi is None:
        return 0, 0, w, h
    return int(roi[0]), int(roi[1]), min(int(roi[2]), w), min(int(roi[3]), h)


# ---------------------------------------------------------------------------------------------- disparity fields
def _smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (100 + x + 2 * y).astype(np.int16), x, y


def f_smooth(w=W, h=H):
    """a smooth valid field, 6.25 .. 20 px: no hole under either Q"""
    return _smooth(w, h)[0]


def f_single_holes(w=W, h=H):
    """isolated single-pixel zero-disparity holes on a 7 x 5 lattice: 1 hole tap at most; an integer position on one is status 1"""
    d, x, y = _smooth(w, h)
    d[(x % 7 == 3) & (y % 5 == 2)] = 0
    return d


def f_hole_blocks(w=W, h=H):
    """2 x 2 zero blocks on a 9 x 8 lattice, a 7 x 7 block and single holes: 0, 1, 2, 3 or 4 hole taps"""
    d, x, y = _smooth(w, h)
    d[(x % 9 < 2) & (y % 8 < 2)] = 0
    d[(x % 9 == 5) & (y % 8 == 5)] = 0
    d[10:17, 40:47] = 0
    return d


def f_hole_band(w=W, h=H):
    """a band of zeros, rows 8 .. 31 x columns 10 .. 59: room for 64 and for 256 consecutive matches that are all status 2"""
    d = _smooth(w, h)[0]
    d[8:32, 10:60] = 0
    return d


def f_invalid(w=W, h=H):
    """pixels at (minDisparity - 1) * 16 = -16 (finite, negative, NOT skipped: they mix into the mean) beside zero holes"""
    d, x, y = _smooth(w, h)
    d[(x % 6 == 1) & (y % 4 == 1)] = INVALID16
    d[(x % 11 == 5) & (y % 7 == 3)] = 0
    return d


def f_w_zero(w=W, h=H):
    """for the Q[3,3] != 0 matrix: d16 = 8 (W = 8 d - 4 == 0) as single pixels and a 3 x 3 block that touches one of them (0 .. 4 hole taps), beside zero disparities (finite there)"""
    d, x, y = _smooth(w, h)
    d[(x % 7 == 3) & (y % 5 == 2)] = 8
    d[(x % 13 == 6) & (y % 9 == 4)] = 0
    d[12:15, 21:24] = 8
    return d


FIELDS = dict(smooth=f_smooth, single_holes=f_single_holes, hole_blocks=f_hole_blocks, hole_band=f_hole_band, invalid=f_invalid, w_zero=f_w_zero)


# ---------------------------------------------------------------------------------------------- the definition, twice
def reproject(disp16, Q, dtype=np.float64):
    """the per-pixel part on the whole image -> (h, w, 3); dtype float64: the definition's roundings, float32 out; np.longdouble: none"""
    disp16 = np.asarray(disp16, np.int16)
    h, w = disp16.shape
    Q = np.asarray(Q, np.float64).astype(dtype)
    d = (disp16.astype(np.float32) / np.float32(16.0)).astype(dtype)          # (exact in float32: |disp16| < 2^15)
    y, x = np.mgrid[0:h, 0:w]
    v = (x.astype(dtype), y.astype(dtype), d, np.ones((h, w), dtype))
    hg = []
    for i in range(4):
        s = np.zeros((h, w), dtype)
        for k in range(4):
            s = s + Q[i, k] * v[k]
        hg.append(s)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ialpha = dtype(1.0) / hg[3]
        if dtype is np.float64:
            out = [(hg[i].astype(np.float32).astype(np.float64) * ialpha).astype(np.float32) for i in range(3)]
        else:
            out = [hg[i] * ialpha for i in range(3)]
    return np.stack(out, 2)


def _taps(roi, w, h, xy):
    x0, y0, x1, y1 = crop(roi, w, h)
    cw, ch = x1 - x0, y1 - y0
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    fx, fy = x.astype(np.int64), y.astype(np.int64)                            # (truncation: positions are >= 0)
    rx, ry = x - fx, y - fy
    tx = np.stack([fx, fx, fx + 1, fx + 1])
    ty = np.stack([fy, fy + 1, fy, fy + 1])
    wt = np.stack([(1 - rx) * (1 - ry), (1 - rx) * ry, rx * (1 - ry), rx * ry])
    exists = (tx < cw) & (ty < ch)
    gx, gy = np.minimum(tx + x0, w - 1), np.minimum(ty + y0, h - 1)           # (a tap that does not exist is never read: any address)
    return cw, ch, fx, fy, wt, exists, gx, gy


def lookup(disp16, Q, roi, xy):
    disp16 = np.asarray(disp16, np.int16)
    h, w = disp16.shape
    img = reproject(disp16, Q)
    cw, ch, fx, fy, wt, exists, gx, gy = _taps(roi, w, h, xy)
    n = len(fx)
    num, den, used = np.zeros((n, 3), np.float32), np.zeros(n, np.float64), np.zeros(n, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(4):
            p = img[gy[k], gx[k]]
            ok = exists[k] & ~np.isinf(p).any(1)
            wf = wt[k].astype(np.float32)
            t = wf[:, None] * p                                               # float32 x float32
            num = np.where(ok[:, None], num + t, num)
            den = np.where(ok, den + wt[k], den)
            used += ok
        out = (num / den.astype(np.float32)[:, None]).astype(np.float32)
    out[used == 0] = np.nan
    status = np.where(used == 0, 2, np.where(np.isnan(out).any(1), 1, 0)).astype(np.uint8)
    return out, status


def exact(disp16, Q, roi, xy):
    """np.longdouble throughout; the taps used are those the definition uses (its float32 image decides what is inf)"""
    disp16 = np.asarray(disp16, np.int16)
    h, w = disp16.shape
    hole = np.isinf(reproject(disp16, Q)).any(2)
    img = reproject(disp16, Q, np.longdouble)
    cw, ch, fx, fy, wt, exists, gx, gy = _taps(roi, w, h, xy)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).astype(np.longdouble)
    rx, ry = xy[:, 0] - fx, xy[:, 1] - fy
    wl = np.stack([(1 - rx) * (1 - ry), (1 - rx) * ry, rx * (1 - ry), rx * ry])
    n = len(fx)
    num, den = np.zeros((n, 3), np.longdouble), np.zeros(n, np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(4):
            ok = exists[k] & ~hole[gy[k], gx[k]]
            p = np.where(ok[:, None], img[gy[k], gx[k]], 0)
            num = num + wl[k][:, None] * p
            den = den + np.where(ok, wl[k], 0)
        return num / den[:, None]


EDGE_NAMES = ("inner", "last_column", "last_row", "corner")


def classify(disp16, Q, roi, xy):
    """-> dict of (n,) arrays: exist (taps inside the crop), holes (existing taps that are skipped), status, edge (index into
    EDGE_NAMES), mixed (the used taps of non-zero weight mix signs in some coordinate), invalid (an existing tap holds INVALID16),
    wzero (an existing tap has W == 0 at a non-zero disparity), and clipped (bool: the image clips the ROI's far edge)"""
    disp16 = np.asarray(disp16, np.int16)
    h, w = disp16.shape
    img = reproject(disp16, Q)
    hole = np.isinf(img).any(2)
    Q = np.asarray(Q, np.float64)
    wz = (Q[3, 2] * (disp16.astype(np.float64) / 16.0) + Q[3, 3] == 0) & (disp16 != 0)
    cw, ch, fx, fy, wt, exists, gx, gy = _taps(roi, w, h, xy)
    th = exists & hole[gy, gx]
    used = exists & ~hole[gy, gx] & (wt > 0)
    p = img[gy, gx]                                                            # (4, n, 3)
    with np.errstate(invalid="ignore"):
        lo = np.where(used[:, :, None], p, np.inf).min(0)
        hi = np.where(used[:, :, None], p, -np.inf).max(0)
    return dict(exist=exists.sum(0), holes=th.sum(0), status=lookup(disp16, Q, roi, xy)[1], edge=(fx + 1 == cw) * 1 + (fy + 1 == ch) * 2,
                mixed=((lo < 0) & (hi > 0)).any(1), invalid=(exists & (disp16[gy, gx] == INVALID16)).any(0), wzero=(exists & wz[gy, gx]).any(0),
                clipped=roi is not None and (roi[2] > w or roi[3] > h))


# ---------------------------------------------------------------------------------------------- position sets
def _below(v):
    return np.nextafter(np.float32(v), np.float32(0))


def _hole_mask(disp16, Q, roi):
    h, w = disp16.shape
    x0, y0, x1, y1 = crop(roi, w, h)
    return np.isinf(reproject(disp16, Q)).any(2)[y0:y1, x0:x1]


def p_integer(disp16, Q, roi, cw, ch, rng, n):
    """integer positions, the last column and row among them"""
    return np.stack([rng.integers(0, cw, n), rng.integers(0, ch, n)], 1)


def p_half(disp16, Q, roi, cw, ch, rng, n):
    """half-integer positions"""
    return np.stack([rng.integers(0, cw, n), rng.integers(0, ch, n)], 1) + 0.5


def p_quarter(disp16, Q, roi, cw, ch, rng, n):
    """k / 4 positions"""
    return np.stack([rng.integers(0, 4 * cw, n), rng.integers(0, 4 * ch, n)], 1) / 4.0


def p_float(disp16, Q, roi, cw, ch, rng, n):
    """arbitrary float32 positions"""
    xy = np.stack([rng.uniform(0, cw, n), rng.uniform(0, ch, n)], 1).astype(np.float32)
    return np.minimum(xy, np.float32([_below(cw), _below(ch)]))


def p_edges(disp16, Q, roi, cw, ch, rng, n):
    """the last column (fx + 1 == cw), the last row (fy + 1 == ch) and the corner, at integer, fractional and largest-below positions"""
    far_x, far_y = (cw - 1, cw - 0.75, cw - 0.5, _below(cw)), (ch - 1, ch - 0.75, ch - 0.5, _below(ch))
    in_x, in_y = (0, 0.5, 7.25, cw - 2, cw - 1.5), (0, 0.5, 7.25, ch - 2, ch - 1.5)
    hm = _hole_mask(disp16, Q, roi)         # ... and beside every hole the field has in that column / row: an edge AND a skipped tap
    holes = [(cw - 0.5, y - 0.5) for y in np.nonzero(hm[:, cw - 1])[0] if y > 0] + [(x - 0.5, ch - 0.5) for x in np.nonzero(hm[ch - 1])[0] if x > 0]
    return np.array([(x, y) for x in far_x for y in in_y] + [(x, y) for x in in_x for y in far_y] + [(x, y) for x in far_x for y in far_y] + holes)


def p_hole_counts(disp16, Q, roi, cw, ch, rng, n):
    """inner positions placed so that exactly 0, 1, 2, 3 or 4 of the four taps are holes (up to 12 of each count the field offers)"""
    hm = _hole_mask(disp16, Q, roi)
    cnt = hm[:-1, :-1] * 1 + hm[1:, :-1] + hm[:-1, 1:] + hm[1:, 1:]
    out = []
    for c in range(5):
        fy, fx = np.nonzero(cnt == c)
        sel = rng.permutation(len(fx))[:12]
        for k, i in enumerate(sel):
            out.append((fx[i] + (0.5, 0.25, 0.8125)[k % 3], fy[i] + (0.5, 0.75, 0.0625)[k % 3]))
    return np.array(out).reshape(-1, 2)


def p_on_hole(disp16, Q, roi, cw, ch, rng, n):
    """integer positions ON a hole, and integer x / half-integer y on two holes stacked: the hole is skipped, every other tap has
    weight 0 but counts as used -- 0 / 0, status 1 -- unless those taps are holes too (status 2)"""
    hm = _hole_mask(disp16, Q, roi)
    fy, fx = np.nonzero(hm)
    sel = rng.permutation(len(fx))[:40]
    out = [(fx[i], fy[i]) for i in sel]
    fy, fx = np.nonzero(hm[:-1] & hm[1:])
    out += [(fx[i], fy[i] + 0.5) for i in rng.permutation(len(fx))[:10]]
    return np.array(out, np.float64).reshape(-1, 2)


POSITIONS = dict(integer=p_integer, half=p_half, quarter=p_quarter, float=p_float, edges=p_edges, hole_counts=p_hole_counts, on_hole=p_on_hole)


def positions(name, disp16, Q, roi, n=300, seed=0):
    """-> (m, 2) float32 inside the crop (m = n for the random sets; what the field offers for the searched ones, possibly 0)"""
    h, w = disp16.shape
    x0, y0, x1, y1 = crop(roi, w, h)
    rng = np.random.default_rng([seed, zlib.crc32(name.encode()), x1 - x0, y1 - y0])
    xy = np.ascontiguousarray(POSITIONS[name](disp16, Q, roi, x1 - x0, y1 - y0, rng, n), np.float32).reshape(-1, 2)
    assert (xy >= 0).all() and (xy[:, 0].astype(np.int64) < x1 - x0).all() and (xy[:, 1].astype(np.int64) < y1 - y0).all(), name
    return xy


def mixed_positions(disp16, Q, roi, n, seed=0):
    """n positions drawn from all the sets together (the sizes of the k_points3d grid tails: 1, 63, 64, 65, 300)"""
    allp = np.concatenate([positions(s, disp16, Q, roi, 200, seed) for s in POSITIONS])
    rng = np.random.default_rng([seed, n])
    return np.ascontiguousarray(allp[rng.permutation(len(allp))[:n]])


COMBOS = [(f, q, r) for f in FIELDS for q in QS for r in ROIS]


# ---------------------------------------------------------------------------------------------- the fused pose step on dense slots
PLANE_ROW = 32                              # image rows above it: the near-half disparity, from it on: twice that
PLANES16 = dict(plain=(128, 256), w33=(136, 264))      # W = 80 | 160 and 64 | 128: a shift of 2 | 4 px is the SAME translation on both planes
SHIFT = (2, 4)


def planes(qname, w=W, h=H):
    """two fronto-parallel disparity planes, one above the other"""
    d = np.empty((h, w), np.int16)
    d[:PLANE_ROW], d[PLANE_ROW:] = PLANES16[qname]
    return d


class DenseCase(P.Case):
    """nq query keypoints of which M must match, on two fronto-parallel planes; slot b's partner of a keypoint is shifted by 2 | 4
    whole pixels (an exact rigid translation of a non-planar cloud).  q / roi: names in QS / ROIS.  holes:
        none       every tap valid, integer positions
        renorm     arbitrary float32 fractions (the partner in b has its keypoint's), the (fx + 1, fy) tap of every third matched
                   keypoint of a is a hole: den < 1 and no power of two
        status1    integer positions, every fifth matched keypoint of a (every seventh of b) sits ON a single hole
        status2    integer positions, every sixth matched keypoint of a has all four taps in a 2 x 2 hole block
        both       status1 and status2
    edge: the partner in b of every second matched keypoint lies in the LAST COLUMN of the crop (fx + 1 == cw) at a fractional position:
    two taps do not exist, the other two are renormalised.
    xyz_a / xyz_b (what the sparse-planted twin carries): lookup() of every keypoint, NaN triples at status 2.  model(): planted.Case's,
    fed with these points;  dense_flags(m): the model's flags plus bit 0 when a MATCHED keypoint has status 2."""

    def __init__(self, name, nq, M, q="plain", roi="none", holes="none", edge=False, **kw):
        super().__init__(name, nq, M, "dense", **kw)
        self.qname, self.roiname, self.holes, self.edge = q, roi, holes, edge

    def build(self):
        if hasattr(self, "disp_a"):
            return self
        rng = np.random.default_rng([self.seed, self.nq, self.M, zlib.crc32(self.name.encode())])
        self.dq, self.dt, q, t = P.descriptors(self.nq, self.M, rng)
        nt = len(self.dt)
        self.Q, self.roi = QS[self.qname], ROIS[self.roiname]
        x0, y0, x1, y1 = crop(self.roi, W, H)
        cw, ch = x1 - x0, y1 - y0
        xa = np.stack([rng.integers(1, cw - 6, self.nq), rng.integers(1, ch - 3, self.nq)], 1)
        xb = np.stack([rng.integers(1, cw - 2, nt), rng.integers(1, ch - 3, nt)], 1)
        shift = np.where(xa[q, 1] + y0 >= PLANE_ROW, SHIFT[1], SHIFT[0])
        if self.edge:
            xa[q[::2], 0] = cw - 1 - shift[::2]
        xb[t] = xa[q] + np.stack([shift, np.zeros(len(q), np.int64)], 1)
        fractional = self.holes == "renorm" or self.edge
        fa, fb = (rng.uniform(0.1, 0.9, (self.nq, 2)), rng.uniform(0.1, 0.9, (nt, 2))) if fractional else (np.zeros((self.nq, 2)), np.zeros((nt, 2)))
        fb[t] = fa[q]
        self.xy_a, self.xy_b = (xa + fa).astype(np.float32), (xb + fb).astype(np.float32)
        self.disp_a, self.disp_b = planes(self.qname), planes(self.qname)
        hole = HOLE16[self.qname]
        ga, gb = xa + (x0, y0), xb + (x0, y0)              # image coordinates of the (fx, fy) taps
        if self.holes == "renorm":
            for k in range(0, len(q), 3):
                self.disp_a[ga[q[k], 1], ga[q[k], 0] + 1] = hole
        if self.holes in ("status1", "both"):
            for k in range(0, len(q), 5):
                self.disp_a[ga[q[k], 1], ga[q[k], 0]] = hole
            for k in range(3, len(q), 7):
                self.disp_b[gb[t[k], 1], gb[t[k], 0]] = hole
        if self.holes in ("status2", "both"):
            for k in range(2, len(q), 6):
                self.disp_a[ga[q[k], 1]:ga[q[k], 1] + 2, ga[q[k], 0]:ga[q[k], 0] + 2] = hole
        self.xyz_a, self.st_a = lookup(self.disp_a, self.Q, self.roi, self.xy_a)
        self.xyz_b, self.st_b = lookup(self.disp_b, self.Q, self.roi, self.xy_b)
        return self

    def dense_flags(self, m):
        return m["counts"][3] | int((self.st_a[m["q"]] == 2).any() or (self.st_b[m["t"]] == 2).any())


F0 = dict(rigidity=0.0)                     # the clique filter off: a NaN point reaches the fit (flag bit 1)
POSE_CASES = [
    DenseCase("all_valid_nq80_M60", 80, 60),
    DenseCase("all_valid_nq300_M280", 300, 280),
    DenseCase("renormalised_taps", 80, 60, holes="renorm"),
    DenseCase("status1_filter_on", 80, 60, holes="status1"),
    DenseCase("status1_filter_off", 80, 60, holes="status1", **F0),
    DenseCase("status2_filter_on", 80, 60, holes="status2"),
    DenseCase("status1_and_2_filter_off", 300, 280, holes="both", **F0),
    DenseCase("last_column_fractional", 80, 60, holes="renorm", edge=True),
    DenseCase("roi_origin_3_5", 80, 60, roi="inner"),
    DenseCase("roi_origin_3_5_last_column", 80, 60, roi="inner", edge=True),
    DenseCase("roi_origin_3_5_status2", 80, 60, roi="inner", holes="status2"),
    DenseCase("roi_clipped", 80, 60, roi="clipped", holes="renorm", edge=True),
    DenseCase("q33_all_valid", 80, 60, q="w33"),
    DenseCase("q33_status1_and_2", 80, 60, q="w33", roi="inner", holes="both"),
]


# ---------------------------------------------------------------------------------------------- the fused PnP step on dense slots
BAND = (10, 8, 40, 30)                      # image columns 10 .. 39 x rows 8 .. 29: all holes (status 2 inside)
LATTICE = (50, 8, 78, 30)                   # single holes every third pixel of this window (status 1 ON one)
FREE_ROW = 34                               # image rows from here on: single holes on a 5 x 4 lattice only -- a keypoint at a fractional position
                                            # there is usable (status 0), one in five with a renormalised tap: the usable keypoints live there


def pnp_field(qname, w=W, h=H):
    d = f_smooth(w, h)
    hole = HOLE16[qname]
    d[BAND[1]:BAND[3], BAND[0]:BAND[2]] = hole
    d[LATTICE[1]:LATTICE[3]:3, LATTICE[0]:LATTICE[2]:3] = hole
    d[FREE_ROW + 1::4, 2::5] = hole
    return d


def _small_motion():
    return P._motion(angle=0.01, t=(0.004, -0.002, 0.01))


class DensePnpCase(PP.PnpCase):
    """planted_pnp.PnpCase (descriptors, duplicates, right descriptors, the model) on a dense slot a: `bad` matches (positions in
    match order) are unusable because of WHERE the keypoint sits -- even ones inside the hole band (status 2), odd ones on a single
    hole (status 1) -- and the usable ones lie at arbitrary float32 positions of the lower rows (a fifth of them beside a single
    hole: renormalised), every tenth of them in the LAST COLUMN of the crop (fx + 1 == cw).  An inlier's partner in b is the
    projection of its looked-up point under a small motion (K4S[q]: the camera the Q describes), minus the ROI origin."""

    def __init__(self, name, nq, M, q="plain", roi="none", **kw):
        super().__init__(name, nq, M, roi=ROIS[roi], **kw)
        self.qname, self.roiname, self.K4 = q, roi, K4S[q]

    def build(self):
        if hasattr(self, "disp_a"):
            return self
        super().build()                     # descriptors, duplicates, right descriptors: the parent's.  Positions and points: below
        q, t, nt = self.q0, self.t0, len(self.dt)
        rng = np.random.default_rng([11, self.scene, self.nq, self.M])
        self.Q = QS[self.qname]
        x0, y0, x1, y1 = crop(self.roi, W, H)
        cw, ch = x1 - x0, y1 - y0
        org = np.array([x0, y0], np.float64)
        self.disp_a, self.disp_b = pnp_field(self.qname), f_smooth()
        free = lambda n: np.stack([rng.uniform(5, min(x1, 80) - 4, n), rng.uniform(FREE_ROW, min(y1, 50) - 2.5, n)], 1) - org   # noqa: E731
        xa = free(self.nq)
        xa[::10, 0] = cw - 1 + rng.uniform(0.1, 0.9, len(xa[::10]))
        for k, p in enumerate(self.bad):
            if k % 2 == 0:
                xa[q[p]] = (rng.uniform(BAND[0], BAND[2] - 1), rng.uniform(BAND[1], BAND[3] - 1)) - org
            else:
                xa[q[p]] = (rng.choice(np.arange(LATTICE[0], LATTICE[2], 3)), rng.choice(np.arange(LATTICE[1], LATTICE[3], 3))) - org
        self.xy_a = xa.astype(np.float32)
        self.xyz_a, self.st_a = lookup(self.disp_a, self.Q, self.roi, self.xy_a)
        xb = np.stack([rng.uniform(0, cw - 1, nt), rng.uniform(0, ch - 1, nt)], 1)
        R, tv = _small_motion()
        fx, fy, cx, cy = self.K4
        with np.errstate(invalid="ignore"):
            Y = self.xyz_a[q[self.inl_pos]].astype(np.float64) @ R.T + tv
            uv = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1) - org + self.noise * rng.normal(0, 1, (len(Y), 2))
        ok = np.isfinite(uv).all(1) & (uv >= 0).all(1) & (uv[:, 0] < cw - 1) & (uv[:, 1] < ch - 1)       # (a partner outside the crop stays where it was drawn)
        xb[t[self.inl_pos[ok]]] = uv[ok]
        self.xy_b = xb.astype(np.float32)
        self.xyz_b, self.st_b = lookup(self.disp_b, self.Q, self.roi, self.xy_b)
        return self


def _pnp_cases():
    kw = dict(noise=0.3)
    scattered = lambda M: [i for i in range(M) if i % 7 in (2, 5)]              # noqa: E731
    return [
        DensePnpCase("M200_all_usable", 203, 200, **kw),
        DensePnpCase("M200_scattered", 203, 200, bad=scattered(200), **kw),
        DensePnpCase("M300_scattered", 305, 300, bad=scattered(300), **kw),
        DensePnpCase("M300_wave1_of_pass0_unusable", 305, 300, bad=range(64, 128), **kw),
        DensePnpCase("M300_pass0_unusable", 305, 300, bad=range(256), **kw),
        DensePnpCase("M40_three_usable", 45, 40, bad=[i for i in range(40) if i not in (3, 17, 30)], n_in=3, **kw),
        DensePnpCase("M300_roi_origin_3_5", 305, 300, roi="inner", bad=scattered(300), **kw),
        DensePnpCase("M300_roi_clipped", 305, 300, roi="clipped", bad=scattered(300), **kw),
        DensePnpCase("M300_q33_roi_origin_3_5", 305, 300, q="w33", roi="inner", bad=scattered(300), **kw),
        DensePnpCase("M300_cross_check", 320, 300, cross=True, dup=30, bad=scattered(300), **kw),
    ]


PNP_CASES = _pnp_cases()
