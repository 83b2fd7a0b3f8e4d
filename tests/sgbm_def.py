"""What a semi-global block matching result MEANS, stated path by path in plain numpy (int64 throughout).

This module imports nothing from oracle/ or openvo_amd/ and shares no code with either.  It is written in another FORM than
oracle/src/sgbm.c (which follows stereosgbm.cpp with its rolling Lr / minLr row buffers, its fused fifth path and its sliding
box sums): every direction's L_r here is a whole (H, W1, D) volume computed by its own recursion from the image border, S is
their sum, the box sum is a sum of shifted copies.  A buffer-reuse slip in that file cannot be inherited here.  Everything is
integer, so whoever is compared with this module is compared for EQUALITY.

Published (H. Hirschmueller, "Stereo Processing by Semiglobal Matching and Mutual Information", PAMI 30(2), 2008):
    eq. 13   L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + P1, L_r(p-r, d+1) + P1, min_i L_r(p-r, i) + P2)
                         - min_k L_r(p-r, k)
    eq. 14   S(p, d) = sum over r of L_r(p, d), 8 (or 16) paths; the disparity is argmin_d S(p, d), sub-pixel by a
             parabola through the neighbouring costs; the match image's disparity "by traversing the epipolar line" from the
             same S, and the consistency check between the two; the uniqueness idea (a margin between the best and
             the next cost) is the OpenCV parameter's documented meaning, not the paper's
    S. Birchfield, C. Tomasi, "Depth Discontinuities by Pixel-to-Pixel Stereo", IJCV 35(3), 1999: the sampling-insensitive
             pixel dissimilarity over half-pixel interpolated neighbours
Published by OpenCV's documentation of cv::StereoSGBM: "single-pass, 5 directions" by default and 8 with MODE_HH; blocks, not
    single pixels; the Birchfield-Tomasi sub-pixel metric; preFilterCap clips the x-derivative to [-cap, cap]; P1 for a change
    of +-1 and P2 for more, P2 > P1; uniquenessRatio as "margin in percentage by which the best (minimum) computed cost
    function value should win the second best value"; disp12MaxDiff; speckleWindowSize / speckleRange (the range "implicitly
    multiplied by 16"); the result is a 16-bit fixed-point disparity with 4 fractional bits; the median blur and
    filterSpeckles' connected components are documented functions of their own.
Recalled from OpenCV's behaviour (stereosgbm.cpp as remembered; the suite has no cv2 to pin them with -- tests/test_cv2_crosscheck.py
    is the place once there is one): the defaults of `effective`; ftzero = max(cap, 15) | 1; the second channel (raw intensity, its
    cost shifted right by 2); ftzero in columns 0 and w - 1 of both channels; the computed band and the clamping of the box sum
    to it; + P2 inside C (it cancels in eq. 13's recursion only where a predecessor exists: at the border a path starts at
    C - P2, i.e. at the bare box sum); the zero vector as the predecessor outside the band; WHICH five directions; the clamp of S
    at 32767 and "every sum saturated = no winner"; first minimum; |d - best| > 1 and the strict `<` of the uniqueness test; the
    tie rule of disp2; the exact integer sub-pixel formula and C's truncation; the two-sided left-right test with its
    `disp2 >= minD` guard over a disp2 that starts at the INVALID value (so for minD >= 2 an unset entry passes the guard).

Stages: effective, planes, cost_volume, path, summed, wta, median3, speckle, compute.  `mut` names ONE deliberately wrong
variant (MUTANTS) for tests/test_sgbm_def.py, which shows that the cases tell each of them from the definition; mut=None is
the definition."""
import collections

import numpy as np

MAX_S = 32767
INF = 1 << 40

# direction name -> r = (dx, dy): the path reaches p from q = p - r, so "W" comes from the west (q = (x - 1, y))
DIRS = {"W": (1, 0), "NW": (1, 1), "N": (0, 1), "NE": (-1, 1), "E": (-1, 0), "SW": (1, -1), "S": (0, -1), "SE": (-1, -1)}
MODE_DIRS = {0: ("W", "NW", "N", "NE", "E"), 1: ("W", "NW", "N", "NE", "E", "SW", "S", "SE")}

MUTANTS = ("lr_one_probe", "uniq_gt0", "uniq_le", "disp2_ge", "subpix_no_den", "subpix_floor", "dceil_16", "p1_one_neighbour",
           "four_paths", "eight_paths", "no_clamp", "last_min", "raw_unshifted", "border_not_ftzero", "box_zero_pad",
           "box_image_clamp")

Eff = collections.namedtuple("Eff", "minD D ur d12 P1 P2 r ftzero x0 x1 W1 invalid window srange")


def effective(params, w):
    """the parameters as vo_set_sgbm derives them, the computed band [x0, x1) and the invalid value"""
    g = params.get
    minD, D = int(params["minDisparity"]), int(params["numDisparities"])
    ur = int(g("uniquenessRatio", -1))
    d12 = int(g("disp12MaxDiff", 0))
    P1 = int(g("P1", 0))
    P2 = int(g("P2", 0))
    bs = int(g("blockSize", 0))
    P1 = P1 if P1 > 0 else 2
    P2 = max(P2 if P2 > 0 else 5, P1 + 1)
    x0, x1 = max(minD + D, 0), w + min(minD, 0)
    return Eff(minD=minD, D=D, ur=ur if ur >= 0 else 10, d12=d12 if d12 > 0 else 1, P1=P1, P2=P2, r=(bs if bs > 0 else 5) // 2,
               ftzero=max(int(g("preFilterCap", 0)), 15) | 1, x0=x0, x1=x1, W1=x1 - x0, invalid=(minD - 1) * 16,
               window=int(g("speckleWindowSize", 0)), srange=int(g("speckleRange", 0)))


def planes(img, ftzero, mut=None):
    """(2, H, w): the x-Sobel clipped to +-ftzero plus ftzero (rows replicated at the top and bottom), and the raw intensity;
    both are ftzero in columns 0 and w - 1"""
    I = np.asarray(img).astype(np.int64)
    h, w = I.shape
    P = np.pad(I, ((1, 1), (0, 0)), mode="edge")
    g = np.zeros((h, w), np.int64)
    for k, wt in ((0, 1), (1, 2), (2, 1)):
        g[:, 1:w - 1] += wt * (P[k:k + h, 2:] - P[k:k + h, :w - 2])
    out = np.stack([np.clip(g, -ftzero, ftzero) + ftzero, I])
    if mut != "border_not_ftzero":
        out[:, :, 0] = ftzero
        out[:, :, w - 1] = ftzero
    return out


def _half_bounds(a):
    """per pixel the least and the greatest of a[x], (a[x] + a[x-1]) / 2, (a[x] + a[x+1]) / 2 (no neighbour beyond the image);
    the values are >= 0, so // is C's truncating division"""
    lo, hi = a.copy(), a.copy()
    half = (a[..., 1:] + a[..., :-1]) // 2             # half[i] lies between pixels i and i + 1
    for sl in (np.s_[..., 1:], np.s_[..., :-1]):         # ... the left neighbour's side of i + 1, the right one's of i
        lo[sl] = np.minimum(lo[sl], half)
        hi[sl] = np.maximum(hi[sl], half)
    return lo, hi


def pixel_cost(L, R, e, xa, xb, mut=None):
    """(H, xb - xa, D): Birchfield-Tomasi both ways, summed over the two channels, at left columns [xa, xb).  Inside the
    computed band x - d never leaves the image; the clip below only acts for the box_image_clamp variant."""
    h, w = np.asarray(L).shape
    U, V = planes(L, e.ftzero, mut), planes(R, e.ftzero, mut)
    out = np.zeros((h, xb - xa, e.D), np.int64)
    xs = np.arange(xa, xb)
    for c in range(2):
        u, v = U[c], V[c]
        u0, u1 = _half_bounds(u)
        v0, v1 = _half_bounds(v)
        shift = 2 if c == 1 and mut != "raw_unshifted" else 0
        for k in range(e.D):
            xr = xs - (e.minD + k)
            if xa == e.x0 and xb == e.x1:
                assert xr.min() >= 0 and xr.max() < w
            xr = np.clip(xr, 0, w - 1)
            uu, vv = u[:, xs], v[:, xr]
            c0 = np.maximum(0, np.maximum(uu - v1[:, xr], v0[:, xr] - uu))
            c1 = np.maximum(0, np.maximum(vv - u1[:, xs], u0[:, xs] - vv))
            out[:, :, k] += np.minimum(c0, c1) >> shift
    return out


def cost_volume(L, R, params, mut=None):
    """C (H, W1, D) = P2 + the (2r + 1)^2 box sum of the pixel cost, indices clamped to the computed band and the image rows"""
    h, w = np.asarray(L).shape
    e = effective(params, w)
    r = e.r
    if mut == "box_image_clamp":
        xa, xb = max(e.x0 - r, 0), min(e.x1 + r, w)
        pix = pixel_cost(L, R, e, xa, xb, mut)
        pix = np.pad(pix, ((r, r), (r - (e.x0 - xa), r - (xb - e.x1)), (0, 0)), mode="edge")
    else:
        pix = pixel_cost(L, R, e, e.x0, e.x1, mut)
        pix = np.pad(pix, ((r, r), (r, r), (0, 0)), mode="constant" if mut == "box_zero_pad" else "edge")
    rows = sum(pix[k:k + h] for k in range(2 * r + 1))
    return sum(rows[:, k:k + e.W1] for k in range(2 * r + 1)) + e.P2


def _step(c, q, P1, P2, mut=None):
    """eq. 13 for a batch of pixels: c, q (n, D) -> L (n, D); q is the predecessor's L_r (zeros where there is none)"""
    m = q.min(axis=1, keepdims=True)
    down = np.full_like(q, INF)
    up = np.full_like(q, INF)
    down[:, 1:] = q[:, :-1] + P1                      # from d - 1; d = -1 is absent
    if mut != "p1_one_neighbour":
        up[:, :-1] = q[:, 1:] + P1                    # from d + 1; d = D is absent
    return c + np.minimum(np.minimum(q, m + P2), np.minimum(down, up)) - m - P2


def path(C, dx, dy, P1, P2, mut=None):
    """L_r as a whole volume for r = (dx, dy), from the border inwards"""
    H, W, D = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        q = np.zeros((H, D), np.int64)
        for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
            q = L[:, x] = _step(C[:, x], q, P1, P2, mut)
        return L
    prev = np.zeros((W, D), np.int64)
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        q = np.zeros((W, D), np.int64)
        if dx > 0:
            q[1:] = prev[:-1]
        elif dx < 0:
            q[:-1] = prev[1:]
        else:
            q = prev
        prev = L[y] = _step(C[y], q, P1, P2, mut)
    return L


def summed(C, mode, P1, P2, mut=None):
    """S = min(sum of the mode's paths, 32767)"""
    names = MODE_DIRS[mode]
    if mode == 0 and mut == "four_paths":
        names = names[:4]
    if mode == 0 and mut == "eight_paths":
        names = MODE_DIRS[1]
    S = sum(path(C, *DIRS[n], P1, P2, mut) for n in names)
    return S if mut == "no_clamp" else np.minimum(S, MAX_S)


def _cdiv(a, b):
    """C's a / b for b > 0"""
    return np.sign(a) * (np.abs(a) // b)


def wta(S, e, w, mut=None, info=None):
    """S (H, W1, D) -> raw disp1 (H, w) int16: winner, uniqueness, disp2 arbitration, sub-pixel step, left-right check.
    info (a dict) receives the counts of what each rule decided."""
    H, W1, D = S.shape
    assert W1 == e.W1 and D == e.D
    ds = np.arange(D)
    minS = S.min(axis=2)
    best = (D - 1 - np.argmin(S[:, :, ::-1], axis=2)) if mut == "last_min" else np.argmin(S, axis=2)
    winner = ~(S == MAX_S).all(axis=2)
    far = np.abs(ds[None, None, :] - best[:, :, None]) > (0 if mut == "uniq_gt0" else 1)
    lhs, rhs = S * (100 - e.ur), (minS * 100)[:, :, None]
    rejected = (((lhs <= rhs) if mut == "uniq_le" else (lhs < rhs)) & far).any(axis=2)
    ok = winner & ~rejected
    ys, xs = np.nonzero(ok)
    X = xs + e.x0
    b = best[ys, xs]
    ms = minS[ys, xs]
    # disp2: per right column x - d of a row the lowest minS, on equal minS the largest x
    disp2 = np.full((H, w), e.invalid, np.int64)
    x2 = X - (b + e.minD)
    order = np.lexsort((X if mut == "disp2_ge" else -X, ms, x2, ys))
    first = np.ones(len(order), bool)
    first[1:] = (ys[order][1:] != ys[order][:-1]) | (x2[order][1:] != x2[order][:-1])
    win = order[first]
    disp2[ys[win], x2[win]] = b[win] + e.minD
    # sub-pixel step
    d1 = b * 16
    mid = (b > 0) & (b < D - 1)
    ym, xm, bm = ys[mid], xs[mid], b[mid]
    sm, s0, sp = S[ym, xm, bm - 1], S[ym, xm, bm], S[ym, xm, bm + 1]
    den = np.maximum(sm + sp - 2 * s0, 1)
    num = (sm - sp) * 16 + (0 if mut == "subpix_no_den" else den)
    d1[mid] += (num // (2 * den)) if mut == "subpix_floor" else _cdiv(num, 2 * den)
    d1 = d1 + e.minD * 16
    # left-right check
    lo, hi = d1 >> 4, (d1 + (16 if mut == "dceil_16" else 15)) >> 4

    def fails(dd):
        xp = X - dd
        inside = (xp >= 0) & (xp < w)
        v = disp2[ys, np.clip(xp, 0, w - 1)]
        return inside & (v >= e.minD) & (np.abs(v - dd) > e.d12)
    f0, f1 = fails(lo), fails(hi)
    drop = (f0 | f1) if mut == "lr_one_probe" else (f0 & f1)
    out = np.full((H, w), e.invalid, np.int64)
    out[ys[~drop], X[~drop]] = d1[~drop]
    if info is not None:
        tied = np.zeros(len(order), bool)                               # candidates of disp2 that meet an equal minS
        same = ~first[1:] & (ms[order][1:] == ms[order][:-1])
        tied[1:] |= same
        tied[:-1] |= same
        info.update(pixels=H * W1, no_winner=int((~winner).sum()), uniqueness=int((winner & rejected).sum()),
                    left_right=int(drop.sum()), disp2_ties=int(tied.sum()),
                    min_twice_apart=int((((S == minS[:, :, None]) & far).any(axis=2) & winner).sum()),
                    subpixel=int(((d1[~drop] & 15) != 0).sum()), valid=int((~drop).sum()))
    return out.astype(np.int16)


def median3(img):
    """numpy.median of the nine replicate-border neighbours"""
    a = np.asarray(img)
    h, w = a.shape
    P = np.pad(a, 1, mode="edge")
    nine = np.stack([P[j:j + h, i:i + w] for j in range(3) for i in range(3)])
    return np.median(nine, axis=0).astype(a.dtype)


def speckle(img, new_val, window, max_diff):
    """components (4-neighbours, |a - b| <= max_diff, neither == new_val) of at most `window` pixels become new_val"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    idx = np.arange(h * w).reshape(h, w)
    live = a != new_val
    eh = live[:, 1:] & live[:, :-1] & (np.abs(a[:, 1:] - a[:, :-1]) <= max_diff)
    ev = live[1:] & live[:-1] & (np.abs(a[1:] - a[:-1]) <= max_diff)
    i = np.concatenate([idx[:, :-1][eh], idx[:-1][ev]])
    j = np.concatenate([idx[:, 1:][eh], idx[1:][ev]])
    n, label = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(h * w, h * w)), directed=False)
    size = np.bincount(label, minlength=n)
    out = np.array(img, copy=True)
    out[(size[label] <= window).reshape(h, w) & live] = new_val
    return out


def post(raw, e):
    """median, then the speckle filter unless its window is 0 -> (median, final)"""
    med = median3(raw)
    return med, (speckle(med, e.invalid, e.window, 16 * e.srange) if e.window > 0 else med)


def compute(L, R, params, mode=0, mut=None, info=None):
    """-> dict(C, S, raw, median, final): every stage of one pair"""
    h, w = np.asarray(L).shape
    e = effective(params, w)
    if e.W1 <= 0:
        raw = np.full((h, w), e.invalid, np.int16)
        C = S = None
    else:
        C = cost_volume(L, R, params, mut)
        S = summed(C, mode, e.P1, e.P2, mut)
        raw = wta(S, e, w, mut, info)
    med, fin = post(raw, e)
    return dict(C=C, S=S, raw=raw, median=med, final=fin)
