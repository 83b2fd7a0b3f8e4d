"""ORB by its published definitions, in plain numpy (int64 / float64): what a result of csrc/orb.hip or oracle/src/orb.c MEANS.

Nothing here is imported from oracle/ or openvo_amd/, and nothing is shaped like their code: FAST is sixteen brute-force arcs (not
the pairwise-min network), Harris is a float64 formula over integer sums, the angle is numpy's atan2, a descriptor bit is a
comparison of two float64 Gaussian-blurred values.  The only project file read is include/vo_orb_pattern.inc, the data table that
tests/test_oracle_independent.py::test_brief_sampling_table_is_the_published_one pins.

    fast_score / corner_scores / nms / candidates     Rosten & Drummond's segment test, 9 of 16, threshold 20; 3x3 suppression
    quotas                                            features per pyramid level, factor 1 / 1.2f, 8 levels
    harris                                            Harris & Stephens' measure over a 7x7 block, with the float32 error bound
    centroid_angle / atan_poly_bound                  Rosin's intensity centroid over the disc of radius 15
    describe_decisions                                rBRIEF (Rublee et al. 2011): bit j is pair j of the table, turned by the angle
    select_decisions                                  retainBest(2 * quota) by FAST score, then retainBest(quota) by Harris
    check                                             all of it against one result dict -> figures; AssertionError otherwise

A definition in float64 cannot decide what a float32 / 8-bit implementation does within its rounding error, so every comparison
here comes with a bound that is derived where it is stated, and what lies inside the bound is counted as undecidable, not as
agreement: the tests cap the undecidable share.  The keyword arguments that default to a published constant (arc=9, k=0.04,
block=7, border=31, threshold=20, strict=True, offsets=disc) exist so that tests/test_orb_def.py can build wrong implementations
from the same parts and show that `check` refuses them."""
import math
import os

import numpy as np

NLEVELS = 8
EDGE = 31
HALF_PATCH = 15
FAST_T = 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the Bresenham circle of radius 3, clockwise from (0, 3) in (dx, dy)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3))


def load_pattern():
    """(256, 4) int64 rows x0, y0, x1, y1 of include/vo_orb_pattern.inc (comments stripped)."""
    text = open(os.path.join(ROOT, "include", "vo_orb_pattern.inc")).read()
    while "/*" in text:
        a = text.index("/*")
        text = text[:a] + text[text.index("*/", a) + 2:]
    v = np.array([int(t) for t in text.replace("\n", " ").split(",") if t.strip()], np.int64)
    assert v.size == 1024, v.size
    return v.reshape(256, 4)


PATTERN = load_pattern()


# ---- FAST-9/16 ------------------------------------------------------------------------------------------------------------------
def fast_score(img, arc=9):
    """The largest t >= 0 such that `arc` contiguous ring pixels are all > I(p) + t or all < I(p) - t; -1 where no t does; -1 in
    the outer 3 pixels.  For one arc the largest t is min(ring - I(p)) - 1 (brighter) or min(I(p) - ring) - 1 (darker)."""
    I = np.asarray(img).astype(np.int64)
    h, w = I.shape
    out = np.full((h, w), -1, np.int64)
    if h < 7 or w < 7:
        return out
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    best = np.full(c.shape, -1, np.int64)
    for s in range(16):
        seg = d[[(s + k) % 16 for k in range(arc)]]
        best = np.maximum(best, np.maximum(seg.min(0), (-seg).min(0)) - 1)
    out[3:h - 3, 3:w - 3] = best
    return out


def corner_scores(img, arc=9, threshold=FAST_T):
    """fast_score where p is a corner (the test holds at t = threshold), 0 elsewhere."""
    s = fast_score(img, arc)
    return np.where(s >= threshold, s, 0)


def nms(score, strict=True):
    """True where the score is positive and strictly greater than all 8 neighbours' scores (outside the image: 0)."""
    s = np.asarray(score).astype(np.int64)
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), np.int64)
    p[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                keep &= (s > nb) if strict else (s >= nb)
    return keep


def candidates(level_img, mask_level=None, arc=9, strict=True, border=EDGE, threshold=FAST_T):
    """-> (x, y, score) int64 arrays in row-major order: the suppression's survivors at least `border` pixels from every edge
    and where the mask is non-zero."""
    sc = corner_scores(level_img, arc, threshold)
    keep = nms(sc, strict)
    h, w = sc.shape
    inside = np.zeros((h, w), bool)
    if h > 2 * border and w > 2 * border:
        inside[border:h - border, border:w - border] = True
    keep &= inside
    if mask_level is not None:
        keep &= np.asarray(mask_level) != 0
    y, x = np.nonzero(keep)
    return x.astype(np.int64), y.astype(np.int64), sc[y, x]


def level_scale(level):
    return np.float32(float(np.float32(1.2)) ** level)


def quotas(nfeatures):
    """Features wanted per level: a geometric series of ratio 1 / 1.2f in float32 that sums to nfeatures; the last level takes
    what is left."""
    f = np.float32(1.0 / float(np.float32(1.2)))
    nd = np.float32(nfeatures) * (np.float32(1) - f) / (np.float32(1) - np.float32(float(f) ** NLEVELS))
    q = []
    for _ in range(NLEVELS - 1):
        q.append(int(np.rint(nd)))
        nd = np.float32(nd * f)
    q.append(max(nfeatures - sum(q), 0))
    return q


# ---- Harris ---------------------------------------------------------------------------------------------------------------------
def harris_sums(level_img, x, y, block=7):
    """Integer sums a, b, c of Ix^2, Iy^2, Ix Iy (3x3 Sobel) over the block x block window centred on each (x, y)."""
    I = np.asarray(level_img).astype(np.int64)
    h, w = I.shape
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    Ix = np.zeros((h, w), np.int64)
    Iy = np.zeros((h, w), np.int64)
    Ix[1:-1, 1:-1] = (I[:-2, 2:] - I[:-2, :-2]) + 2 * (I[1:-1, 2:] - I[1:-1, :-2]) + (I[2:, 2:] - I[2:, :-2])
    Iy[1:-1, 1:-1] = (I[2:, :-2] - I[:-2, :-2]) + 2 * (I[2:, 1:-1] - I[:-2, 1:-1]) + (I[2:, 2:] - I[:-2, 2:])
    r = block // 2
    a = np.zeros(len(x), np.int64)
    b = np.zeros(len(x), np.int64)
    c = np.zeros(len(x), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            gx, gy = Ix[y + dy, x + dx], Iy[y + dy, x + dx]
            a += gx * gx
            b += gy * gy
            c += gx * gy
    return a, b, c


def harris(level_img, x, y, k=0.04, block=7):
    """-> (value, bound), float64 arrays.  value = (a b - c^2 - k (a + b)^2) * (1 / (4 * block * 255))^4.

    bound is what a float32 evaluation of that expression may differ by.  Every float32 operation returns its exact result times
    (1 + e) with |e| <= 2^-24 (half an ulp, relative).  The expression is a signed sum of three non-negative terms, a b, c^2 and
    k (a + b)^2, and each rounding -- of an integer sum above 2^24 on conversion, of a product, of a + b, of k itself, of a
    difference, of the final scaling -- perturbs a quantity whose magnitude is at most S = a b + c^2 + k (a + b)^2 by at most
    2^-24 of it.  Eight such roundings are allowed for, so bound = 8 * 2^-24 * S * scale^4.  (Counting every rounding on the
    longest chain, k (a + b)^2, as if all were extreme and aligned gives a few more; the tests print the worst error seen as a
    share of this bound, and it has stayed below one half.)"""
    a, b, c = (v.astype(np.float64) for v in harris_sums(level_img, x, y, block))
    s4 = (1.0 / (4 * block * 255.0)) ** 4
    value = (a * b - c * c - k * (a + b) ** 2) * s4
    bound = 8 * 2.0 ** -24 * (a * b + c * c + k * (a + b) ** 2) * s4
    return value, bound


# ---- orientation ----------------------------------------------------------------------------------------------------------------
def disc_offsets(half=HALF_PATCH):
    """(u, v) of every pixel of the patch: |v| <= half, |u| <= umax[|v|], where umax[v] = round(sqrt(half^2 - v^2)) up to the
    45-degree row and the mirror image of those rows beyond it, so that the disc is symmetric under a quarter turn."""
    vmax = int(math.floor(half * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(half * math.sqrt(2.0) / 2))
    umax = [0] * (half + 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(half * half - v * v)))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    pts = [(u, v) for v in range(-half, half + 1) for u in range(-umax[abs(v)], umax[abs(v)] + 1)]
    return np.array(pts, np.int64)


def square_offsets(half=HALF_PATCH):
    return np.array([(u, v) for v in range(-half, half + 1) for u in range(-half, half + 1)], np.int64)


def moments(level_img, x, y, offsets=None):
    """-> (m10, m01) = (sum u I, sum v I) over the patch, int64."""
    I = np.asarray(level_img).astype(np.int64)
    off = disc_offsets() if offsets is None else offsets
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    P = I[y[:, None] + off[None, :, 1], x[:, None] + off[None, :, 0]]
    return (P * off[None, :, 0]).sum(1), (P * off[None, :, 1]).sum(1)


def centroid_angle(level_img, x, y, offsets=None):
    """atan2(m01, m10) in degrees in [0, 360)."""
    m10, m01 = moments(level_img, x, y, offsets)
    return np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0


ATAN_POLY = (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)


def atan_poly_bound():
    """Degrees: the worst deviation of the published degree-7 odd polynomial (fastAtan2's) from atan on [0, 1], on 1e5 points in
    float64, plus 5e-4 degrees for its float32 evaluation (a handful of roundings of values up to 360, ulp 3e-5)."""
    c = np.linspace(0.0, 1.0, 100000)
    c2 = c * c
    p = (((ATAN_POLY[3] * c2 + ATAN_POLY[2]) * c2 + ATAN_POLY[1]) * c2 + ATAN_POLY[0]) * c
    return float(np.abs(np.degrees(p) - np.degrees(np.arctan(c))).max()) + 5e-4


def angle_diff(a, b):
    """|a - b| on the circle, degrees."""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


# ---- descriptor -----------------------------------------------------------------------------------------------------------------
K0 = np.array([18, 34, 49, 55, 49, 34, 18], np.float64)     # float kernel * 256, rounded
K1 = np.array([18, 34, 48, 56, 48, 34, 18], np.float64)     # error-diffused fixed point, sums to 256
HALF_TOL = 1e-3


def gauss7():
    g = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / (2 * 2.0 ** 2))
    g /= g.sum()
    return np.outer(g, g)


def _correlate7(I, K):
    h, w = I.shape
    P = np.pad(I, 3, mode="reflect")
    out = np.zeros((h, w), np.float64)
    for j in range(7):
        for i in range(7):
            out += K[j, i] * P[j:j + h, i:i + w]
    return out


def blur_and_bound(level_img):
    """-> (B, E): the float64 Gaussian blur (7x7, sigma 2, normalised, reflected border) and, per pixel, how far an 8-bit blur
    with either of the two fixed-point kernels may lie from it: sum over taps of I * max |k (x) k / 65536 - G|, plus 0.5 for the
    rounding to 8 bits (saturation at 255 only moves towards B, which never exceeds 255)."""
    I = np.asarray(level_img).astype(np.float64)
    G = gauss7()
    D = np.maximum(np.abs(np.outer(K0, K0) / 65536.0 - G), np.abs(np.outer(K1, K1) / 65536.0 - G))
    return _correlate7(I, G), _correlate7(I, D) + 0.5


def turn(angle_deg, negate_sin=False, shift_rows=0):
    """The table's 512 points turned by each angle: (x cos - y sin, x sin + y cos), float64, shape (n, 256) each."""
    a = np.radians(np.asarray(angle_deg, np.float64))[:, None]
    ca, sa = np.cos(a), (-np.sin(a) if negate_sin else np.sin(a))
    T = np.roll(PATTERN, shift_rows, axis=0).astype(np.float64)
    x0, y0, x1, y1 = (T[None, :, i] for i in range(4))
    return x0 * ca - y0 * sa, x0 * sa + y0 * ca, x1 * ca - y1 * sa, x1 * sa + y1 * ca


def near_half(v):
    """True where v lies within HALF_TOL of a half-integer: its rounding is not decided by the definition."""
    return np.abs((v - np.floor(v)) - 0.5) <= HALF_TOL


def describe_decisions(level_img, x, y, angle_deg, blurred=None):
    """-> (bits, decidable), bool (n, 256).  bits[:, j]: the blurred value at the first turned point of pair j is smaller than at
    the second.  decidable[:, j] is False when a turned coordinate is within 1e-3 of a half-integer, or when the two blurred
    values differ by no more than the sum of their bounds (blur_and_bound)."""
    B, E = blur_and_bound(level_img) if blurred is None else blurred
    x, y = np.asarray(x, np.int64)[:, None], np.asarray(y, np.int64)[:, None]
    X0, Y0, X1, Y1 = turn(angle_deg)
    tie = near_half(X0) | near_half(Y0) | near_half(X1) | near_half(Y1)
    ix0, iy0, ix1, iy1 = (np.rint(v).astype(np.int64) for v in (X0, Y0, X1, Y1))
    v0, v1 = B[y + iy0, x + ix0], B[y + iy1, x + ix1]
    e = E[y + iy0, x + ix0] + E[y + iy1, x + ix1]
    return v0 < v1, ~tie & (np.abs(v0 - v1) > e)


def unpack_bits(desc):
    """(n, 32) uint8 -> (n, 256) bool, bit k of byte j being pair 8 j + k."""
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little").astype(bool)


def pack_bits(bits):
    return np.packbits(np.asarray(bits, bool), axis=1, bitorder="little")


# ---- selection ------------------------------------------------------------------------------------------------------------------
def select_decisions(score, value, bound, quota, rank_shift=0):
    """The per-level rule on candidates with FAST scores `score` and float64 Harris (value, bound) -> (must_in, must_out).

    More than 2 * quota candidates: only those whose score is >= the (2 * quota)-th largest go on (ties kept).  Of those, the
    final set is every candidate whose Harris value is >= the quota-th largest (ties kept); no more than quota of them: all.
    A candidate is surely in when its value exceeds the quota-th value by more than its bound plus that value's bound, surely out
    when it falls short by more than both (or lost on the integer score), undecided otherwise."""
    score, value, bound = np.asarray(score, np.int64), np.asarray(value, np.float64), np.asarray(bound, np.float64)
    n = len(score)
    if quota <= 0:
        return np.zeros(n, bool), np.ones(n, bool)
    first = np.ones(n, bool)
    if n > 2 * quota:
        first = score >= np.sort(score)[::-1][2 * quota - 1 + rank_shift]
    must_in, must_out = first.copy(), ~first
    idx = np.nonzero(first)[0]
    if len(idx) > quota:
        v, b = value[idx], bound[idx]
        q = np.argsort(-v, kind="stable")[quota - 1 + rank_shift]
        must_in[idx] = v - v[q] > b + b[q]
        must_out[idx] = v[q] - v > b + b[q]
    return must_in, must_out


# ---- the whole result -----------------------------------------------------------------------------------------------------------
def prepare(levels):
    """Everything of `levels` = [(image, mask or None)] * 8 that does not depend on the request or the result."""
    if isinstance(levels, dict):
        return levels
    per = []
    for img, m in levels:
        img = np.asarray(img)
        h, w = img.shape
        x, y, sc = candidates(img, m)
        val, bnd = harris(img, x, y)
        per.append(dict(img=img, mask=m, w=w, h=h, x=x, y=y, score=sc, value=val, bound=bnd, angle=centroid_angle(img, x, y),
                        blurred=blur_and_bound(img) if len(x) else None))
    return dict(per=per)


def check(result, img, mask, nfeatures, levels):
    """Hold a result dict (xy, size, angle, response, octave, desc) to the definitions -> figures.  levels[0] is (img, mask);
    levels >= 1 are the caller's pyramid and mask levels."""
    P = prepare(levels)["per"]
    assert len(P) == NLEVELS
    assert np.array_equal(P[0]["img"], np.asarray(img)), "level 0 is the input itself"
    assert (mask is None) == (P[0]["mask"] is None) and (mask is None or np.array_equal(P[0]["mask"], mask)), "level 0's mask is the input's"
    xy, octave = np.asarray(result["xy"]), np.asarray(result["octave"]).astype(np.int64)
    n = len(octave)
    for name, shape, dt in (("xy", (n, 2), np.float32), ("size", (n,), np.float32), ("angle", (n,), np.float32),
                            ("response", (n,), np.float32), ("desc", (n, 32), np.uint8)):
        assert np.asarray(result[name]).shape == shape and np.asarray(result[name]).dtype == dt, name
    assert n == 0 or (octave.min() >= 0 and octave.max() < NLEVELS), "octave out of range"
    scale = np.array([level_scale(l) for l in range(NLEVELS)], np.float32)[octave]
    kx = np.rint(xy[:, 0].astype(np.float64) / scale).astype(np.int64)
    ky = np.rint(xy[:, 1].astype(np.float64) / scale).astype(np.int64)
    assert np.array_equal(xy[:, 0], kx.astype(np.float32) * scale) and np.array_equal(xy[:, 1], ky.astype(np.float32) * scale), \
        "xy is not float32(level coordinate) * scale"
    assert np.array_equal(np.asarray(result["size"]), np.float32(31) * scale), "size is not 31 * scale"
    key = (octave * (1 << 20) + ky) * (1 << 20) + kx
    assert (np.diff(key) > 0).all(), "keypoints are not in strict (octave, y, x) order"
    ang = np.asarray(result["angle"]).astype(np.float64)
    assert ((ang >= 0) & (ang < 360)).all(), "angle outside [0, 360)"
    bits = unpack_bits(result["desc"])
    q = quotas(nfeatures)
    abound = atan_poly_bound()
    fig = dict(n=n, per_level=[0] * NLEVELS, candidates=[len(p["x"]) for p in P], quotas=q, bits=0, bits_undecidable=0,
               bits_tie=0, harris_share=0.0, angle_err=0.0, angle_bound=abound, select_undecidable=0, decided_out=0, excess=0)
    fig["set_equality"] = all(c <= k for c, k in zip(fig["candidates"], q))
    for l, p in enumerate(P):
        sel = np.nonzero(octave == l)[0]
        fig["per_level"][l] = len(sel)
        if len(sel):
            assert p["w"] > 2 * EDGE and p["h"] > 2 * EDGE, "keypoints at level %d of %dx%d" % (l, p["w"], p["h"])
        cidx = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(p["x"], p["y"]))}
        at = np.array([cidx.get((int(a), int(b)), -1) for a, b in zip(kx[sel], ky[sel])], np.int64)
        assert (at >= 0).all(), "level %d: %d keypoints are no FAST-9/16 corner that survives suppression, border and mask, " \
            "e.g. (%d, %d)" % (l, int((at < 0).sum()), kx[sel][at < 0][0], ky[sel][at < 0][0])
        present = np.zeros(len(p["x"]), bool)
        present[at] = True
        must_in, must_out = select_decisions(p["score"], p["value"], p["bound"], q[l])
        assert not (must_in & ~present).any(), "level %d: %d candidates the selection rule keeps are missing (quota %d of %d)" \
            % (l, int((must_in & ~present).sum()), q[l], len(present))
        assert not (must_out & present).any(), "level %d: %d keypoints the selection rule drops are present (quota %d of %d)" \
            % (l, int((must_out & present).sum()), q[l], len(present))
        fig["select_undecidable"] += int((~must_in & ~must_out).sum())
        fig["decided_out"] += int(must_out.sum())
        fig["excess"] += max(len(present) - q[l], 0)
        if not len(sel):
            continue
        err = np.abs(np.asarray(result["response"])[sel].astype(np.float64) - p["value"][at])
        share = err / np.maximum(p["bound"][at], 1e-300)
        assert (err <= p["bound"][at]).all(), "level %d: response is not the Harris measure: worst error %.3g of its bound at " \
            "(%d, %d)" % (l, share.max(), kx[sel][share.argmax()], ky[sel][share.argmax()])
        fig["harris_share"] = max(fig["harris_share"], float(share.max()))
        aerr = angle_diff(ang[sel], p["angle"][at])
        assert (aerr <= abound).all(), "level %d: angle is not the intensity centroid's direction: worst error %.4f deg " \
            "(bound %.4f) at (%d, %d)" % (l, aerr.max(), abound, kx[sel][aerr.argmax()], ky[sel][aerr.argmax()])
        fig["angle_err"] = max(fig["angle_err"], float(aerr.max()))
        want, decidable = describe_decisions(p["img"], kx[sel], ky[sel], ang[sel], p["blurred"])
        wrong = decidable & (want != bits[sel])
        assert not wrong.any(), "level %d: %d decidable descriptor bits differ from the published comparison, first at keypoint " \
            "(%d, %d) pair %d" % (l, int(wrong.sum()), kx[sel][np.nonzero(wrong)[0][0]], ky[sel][np.nonzero(wrong)[0][0]],
                                  np.nonzero(wrong)[1][0])
        X = turn(ang[sel])
        fig["bits"] += decidable.size
        fig["bits_undecidable"] += int((~decidable).sum())
        fig["bits_tie"] += int((near_half(X[0]) | near_half(X[1]) | near_half(X[2]) | near_half(X[3])).sum())
    fig["undecidable_share"] = fig["bits_undecidable"] / fig["bits"] if fig["bits"] else 0.0
    return fig


def figures_line(what, f):
    return "%s: %d keypoints %s of candidates %s (quotas %s), bits undecidable %.3f (ties %.4f), Harris error %.3f of its bound, " \
           "angle error %.5f deg (bound %.5f), selection: %d undecided, %d decided out" % (
               what, f["n"], f["per_level"], f["candidates"], f["quotas"], f["undecidable_share"],
               f["bits_tie"] / f["bits"] if f["bits"] else 0.0, f["harris_share"], f["angle_err"], f["angle_bound"],
               f["select_undecidable"], f["decided_out"])
