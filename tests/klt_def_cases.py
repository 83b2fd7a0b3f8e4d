"""The cases at which the Lucas-Kanade kernels are held to tests/klt_def.py: shapes and contents where a kernel can go wrong and the
textures of tests/klt_cases.py cannot show it.  One registry (`cases()`), used alike by tests/test_klt_def.py (the restatement's answer,
on the CPU) and tests/test_gpu_klt_definitions.py (the device's): a case is the two images, the points and the parameters of ONE
vo_klt_track_host call, and `hold` says what its result is held to.  Every cap is asserted on the definition alone, in `caps`,
before a result is looked at.

TAU (px): whole tracks are compared with klt_def.track_def within TAU = 4 x the largest distance between track_def and the
restatement over the tracked points of the smooth whole-track cases, measured on the CPU (TAU_BASIS; test_klt_def.py re-measures
it).  The two differ only by quantisation, whose effect on a fixed point of the iteration has no closed form: hence a measured
figure with a factor, never the kernel's."""
import numpy as np

import klt_cases as C
import klt_def as D

TAU_BASIS = 0.0080                  # px: measured (test_klt_def.py::test_tau_is_four_times_the_measured_distance)
TAU = 4 * TAU_BASIS
BEYOND_CAP = 0.05                   # share of the corridor's tracked points that may lie beyond TAU
UNDECIDABLE_CAP = 0.05              # share of a one-step case's starts the bound may leave undecided (a 5 x 5 window on the smooth texture,
                                    # whose shortest period is 18 px, can see next to no gradient in one direction); a definition whose G
                                    # has rank 1 everywhere (Dy = Dx) leaves every start undecided
STEP = dict(levels=1, iters=1, eps=0.0, min_eig=0.0, fb=0.0)

# ---- pyramid shapes: tile edges of k_klt_pyr_down (32 outputs from 67 source columns, 8 rows from 19) on awkward sizes, sides < 3 -----
PYR_SHAPES = ((1, 1), (2, 3), (3, 2), (4, 15), (5, 17), (31, 16), (32, 33), (33, 1), (63, 17), (64, 16), (65, 33), (66, 3), (67, 15), (129, 2),
              (129, 33))
PYR_LEVELS = 6


def pyr_images(w, h):
    """white noise, and a 0 / 255 pattern: odd columns 255 on the upper half (the taps 4 + 4 of 16 carry exactly half the weight:
    (v + 128) >> 8 meets 127.5 at every such output), random 0 / 255 below"""
    rng = np.random.default_rng(1000 * w + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    pat = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    top = (h + 1) // 2
    pat[:top] = 0
    pat[:top, 1::2] = 255
    return noise, pat


def tie_share(img, levels=PYR_LEVELS):
    """the share of the output pixels of the pyramid above img whose unrounded value is an exact half (on the definition alone)"""
    d = D.Definition()
    ties = total = 0
    lvl = np.asarray(img, np.float64)
    k = np.array([1, 4, 6, 4, 1]) / 16.0
    for _ in range(levels - 1):
        I = lvl
        for axis in (0, 1):
            n = I.shape[axis]
            P = d._pad2(I, axis)
            I = np.take(sum(k[j] * np.take(P, np.arange(j, j + n), axis=axis) for j in range(5)), np.arange(0, n, 2), axis=axis)
        ties += int((I - np.floor(I) == 0.5).sum())
        total += I.size
        lvl = d.pyr_down(lvl)
    return ties / float(total)


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


# ---- points ------------------------------------------------------------------------------------------------------------------------
def dyadic_starts(w, h, n=64, seed=21):
    """n starts with three fractional bits (exact in float32 and in the definition) inside the image: every corner, points within
    2 px of every border, then random ones"""
    sp = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1.125, 0.5), (w - 2.25, h - 1.5), (0.375, h - 1.875), (w - 1.625, 1.25),
          (w * 0.5, 0.25), (w * 0.5, h - 1.25), (0.75, h * 0.5), (w - 1.5, h * 0.5), (1.875, 1.875), (w - 2.875, h - 2.875)]
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.integers(0, 8 * (w - 1) + 1, n), rng.integers(0, 8 * (h - 1) + 1, n)], 1) / 8.0
    xy = np.concatenate([np.floor(np.array(sp, np.float64) * 8) / 8, rnd])[:n]
    return np.clip(xy, 0, [w - 1, h - 1]).astype(np.float32)


def around(w, h, seed=4):
    """16 sub-pixel points inside and just around a (small) image"""
    rng = np.random.default_rng(seed)
    fixed = [(0.0, 0.0), (w - 1.0, h - 1.0), (w * 0.5, h * 0.5), (-1.5, h * 0.5), (w * 0.5, h + 0.75), (w + 1.25, -0.5)]
    rnd = np.stack([rng.uniform(-1, w, 10), rng.uniform(-1, h, 10)], 1)
    return np.concatenate([np.array(fixed), rnd]).astype(np.float32)


# ---- contents ----------------------------------------------------------------------------------------------------------------------
def smooth_small(w, h, shift=(0.6, -0.4)):
    import klt_ref as K
    return K.smooth_texture(w, h, seed=C.SMOOTH_SEED, fmax=0.9), K.smooth_texture(w, h, shift, seed=C.SMOOTH_SEED, fmax=0.9)


def stripes(kind, w=64, h=48):
    """0, 0, 255, 255 stripes: |Scharr| = 16 x 255 = 4080 at every pixel across them.  v: vertical, h: the same turned a quarter,
    d: diagonal (Dx = Dy: A12 = A11), p: the two crossed (a plaid of 2 x 2 blocks: the only one of the four whose G has rank 2)"""
    y, x = np.mgrid[0:h, 0:w]
    on = {"v": x % 4 >= 2, "h": y % 4 >= 2, "d": (x + y) % 4 >= 2, "p": (x % 4 >= 2) ^ (y % 4 >= 2)}[kind]
    return (on * 255).astype(np.uint8)


def extreme_pair(kind, other):
    """other = inverse: B = 255 - A (half a period away: b vanishes by symmetry, up to one window column);  shift: B = A moved one
    pixel along x (y for h), a quarter period: every product (J - I) Dx has one sign and b1 is as large as it can get"""
    a = stripes(kind)
    if other == "inverse":
        return a, (255 - a).astype(np.uint8)
    return a, np.ascontiguousarray(np.roll(a, 1, axis=0 if kind == "h" else 1))


def extreme_starts():
    """12 starts whose 31 x 31 window and its gradient taps lie inside the 64 x 48 stripes"""
    rng = np.random.default_rng(8)
    xy = np.stack([rng.integers(17, 47, 12), rng.integers(17, 31, 12)], 1).astype(np.float64)
    xy[4:8, 0] += 0.125             # (an eighth off on ONE axis: off on both, the diagonal and the plaid fall under 2^32)
    xy[8:, 1] -= 0.125
    return xy.astype(np.float32)


def sums(a, b, xy, win):
    """A11, A12, A22, b1, b2 of the FIRST iteration at level 0 of the definition, in the kernel's units -> (n, 5)"""
    d = D.Definition()
    A, B = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.asarray(xy, np.float64).reshape(-1, 2)
    T = d.template(A, d.gradients(A), c, win)
    J, _ = d.sample(B, 0, c[:, 0], c[:, 1], win)
    dI = 32.0 * J - T["I"]
    return np.stack([T["G11"], T["G12"], T["G22"], (dI * T["Dx"]).sum((1, 2)), (dI * T["Dy"]).sum((1, 2))], 1)


def lane_sum_bound(win=31):
    """the largest |partial sum| a lane of k_klt_track can hold: window pixel p = 64 t + lane, so lane 0 sees ceil(win^2 / 64) pixels,
    each product at most (255 x 32) x 4080 for b and 4080^2 for G"""
    per_lane = -(-win * win // 64)
    return per_lane * 255 * 32 * 4080, per_lane * 4080 * 4080


def eig_images():
    """64 x 48: an edge (every gradient along x: G has rank 1, D = 0) and a corner (one bright quadrant)"""
    edge = np.full((48, 64), 50, np.uint8)
    edge[:, 32:] = 200
    corner = np.full((48, 64), 50, np.uint8)
    corner[24:, 32:] = 200
    return edge, corner


# ---- the registry --------------------------------------------------------------------------------------------------------------------
def _case(kind, name, a, b, xy, **prm):
    return dict(kind=kind, name=name, a=np.ascontiguousarray(a, np.uint8), b=np.ascontiguousarray(b, np.uint8),
                xy=np.ascontiguousarray(xy, np.float32).reshape(-1, 2), prm=prm)


_CASES = []


def cases():
    """every call, in a fixed order (built once)"""
    if _CASES:
        return _CASES
    out = _CASES
    # the pyramid: one call per shape, levels read back; the call's own result is not the point
    for w, h in PYR_SHAPES:
        n, p = pyr_images(w, h)
        out.append(_case("pyr", "pyr-%dx%d" % (w, h), n, p, [(w * 0.5, h * 0.5)], win=5, levels=PYR_LEVELS, fb=0.0))
    fa, fb_, _ = C.fixture()
    sa, sb = C.smooth_pair(96, 64, flat=False)
    # one step, every kernel instantiation (trips 1 .. 2: 5, 7, 9; 3 .. 4: 13; 5 .. 7: 19, 21; 8 .. 10: 25; 11 .. 16: 31)
    for tex, (a, b) in (("corridor", (fa, fb_)), ("smooth", (sa, sb))):
        for win in (5, 7, 9, 13, 19, 21, 25, 31):
            out.append(_case("step", "step-%s-win%d" % (tex, win), a, b, dyadic_starts(a.shape[1], a.shape[0]), win=win, **STEP))
    # ... and on the upper levels of the corridor pair as level-0 images: small and odd shapes through the step arithmetic
    d = D.Definition()
    la, lb = d.pyramid(fa, 4), d.pyramid(fb_, 4)
    for L, wins in ((1, (5, 21)), (2, (9, 31)), (3, (5, 9))):
        for win in wins:
            a, b = la[L].astype(np.uint8), lb[L].astype(np.uint8)
            out.append(_case("step", "step-level%d-win%d" % (L, win), a, b, dyadic_starts(a.shape[1], a.shape[0], 32), win=win, **STEP))
    # images narrower than the window
    for w, h in ((4, 40), (40, 4), (3, 3), (1, 1)):
        a, b = smooth_small(w, h)
        for win in (5, 31):
            for levels in (1, 3):
                out.append(_case("narrow", "narrow-%dx%d-win%d-l%d" % (w, h, win, levels), a, b, around(w, h), win=win, levels=levels, fb=1.0))
    # extremes: windows wholly inside the image (a clamped read is flat), starts on whole pixels and an eighth off them
    ex = extreme_starts()
    for kind in "vhdp":
        for other in ("inverse", "shift"):
            a, b = extreme_pair(kind, other)
            for win in (31, 5):
                out.append(_case("extreme", "extreme-%s-%s-win%d" % (kind, other, win), a, b, ex, win=win, levels=1,
                                 min_eig=0.1 if kind != "p" else 1e-4, fb=0.0))
                if kind == "p":     # the only pair whose G has rank 2: its first step, with every sum at its largest, under the derived bound
                    out.append(_case("step", "step-extreme-p-%s-win%d" % (other, win), a, b, ex, win=win, **STEP))
    a, b = extreme_pair("p", "shift")
    out.append(_case("extreme", "extreme-p-shift-win31-l2", a, b, ex, win=31, levels=2, fb=1.0))
    # the eigenvalue rule: min_eig on both sides of the definitional value
    edge, corner = eig_images()
    fl = C.smooth_pair(96, 64)
    F = C.flat_rect(96, 64)
    flat_xy = [(F[0] + F[2] / 2.0 + dx, F[1] + F[3] / 2.0 + dy) for dx, dy in ((0, 0), (0.25, -0.5), (-1.5, 1.125))]
    cxy = [(32.0 + dx, 24.0 + dy) for dx, dy in ((0, 0), (0.5, 0.25), (-1.25, 1.0), (2.0, -1.5))]
    T = d.template(corner.astype(np.float64), d.gradients(corner.astype(np.float64)), np.array(cxy), 9)
    me = T["lmin"] * 2.0 ** -20 / 81.0
    for tag, f in (("below", 0.75), ("above", 1.25)):
        out.append(_case("eig", "eig-corner-%s" % tag, corner, corner, cxy[:1], win=9, levels=1, min_eig=float(me[0] * f), fb=0.0))
    out.append(_case("eig", "eig-corner-between", corner, corner, cxy, win=9, levels=1, min_eig=float(np.sqrt(me.min() * me.max())), fb=0.0))
    for nm, img, xy in (("edge", edge, cxy), ("flat", fl[0], flat_xy)):
        T = d.template(img.astype(np.float64), d.gradients(img.astype(np.float64)), np.array(xy), 9)
        hi = float(2.0 * ((T["lmin"] + T["dG"]) * 2.0 ** -20 / 81.0).max() + 1e-12)
        out.append(_case("eig", "eig-%s-above" % nm, img, img if nm == "edge" else fl[1], xy, win=9, levels=1, min_eig=hi, fb=0.0))
        out.append(_case("eig", "eig-%s-zero" % nm, img, img if nm == "edge" else fl[1], xy, win=9, levels=1, min_eig=0.0, fb=0.0))
    # whole tracks
    for w, h, win, levels in ((160, 120, 9, 2), (160, 120, 21, 3), (160, 120, 31, 4)):
        for tex, (a, b) in (("smooth", C.smooth_pair(w, h)), ("corridor", C.corridor_pair(w, h))):
            out.append(_case("track", "track-%s-win%d-l%d" % (tex, win, levels), a, b, C.points(w, h, 120, extra=C.fixture()[2]), win=win, levels=levels, fb=1.0))
    out.append(_case("track", "track-osc", fa, fb_, C.fixture()[2], fb=0.0, **C.OSC_PARAMS))
    # ... and points that END level 0 by the oscillation stop with a step of more than 4 TAU (picked on the definition): half a step back
    # and a whole one then lie 2 TAU apart
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(2, 157, 1600), rng.uniform(2, 117, 1600)], 1).astype(np.float32)
    R = d.track_def(fa, fb_, xy, win=5, levels=1, fb=0.0)
    osc = (R["status"] == 0) & R["decided"] & (R["margin"] > TAU) & (R["osc_step"] > 4 * TAU)
    assert osc.sum() >= 40          # (enough for the 5 % cap to allow a point or two: a track that ends by this stop is the least stable there is)
    out.append(_case("track", "track-osc-level0", fa, fb_, xy[osc][:64], win=5, levels=1, fb=0.0))
    # forward-backward: fb just below and just above one point's definitional round trip
    xy = C.points(160, 120, 120)
    R = d.track_def(fa, fb_, xy, win=21, levels=3, fb=1.0e6)
    rt = np.where((R["status"] == 0) & R["decided"] & (R["margin"] > TAU), R["round_trip"], np.nan)
    pick = int(np.nanargmax(np.where(rt < 2.0, rt, np.nan)))
    for tag, f in (("below", 0.75), ("above", 1.25)):
        c = _case("fb", "fb-%s" % tag, fa, fb_, xy, win=21, levels=3, fb=float(rt[pick] * f))
        c["pick"], c["round_trip"] = pick, float(rt[pick])
        out.append(c)
    return out


def by_kind(kind):
    return [c for c in cases() if c["kind"] == kind]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


# ---- caps, on the definition alone ---------------------------------------------------------------------------------------------------
def caps(case):
    """what a case must be BEFORE any result is looked at -> figures; AssertionError where a case does not reach its regime"""
    k, prm = case["kind"], case["prm"]
    d = D.Definition()
    if k == "step":
        p0 = case["xy"].astype(np.float64)
        _, bound = d.step(case["a"], case["b"], p0, p0, prm["win"])
        und = float((~np.isfinite(bound)).mean())
        assert und <= UNDECIDABLE_CAP, "%s: %.3f of the starts are undecidable" % (case["name"], und)
        return dict(undecidable=und)
    if k == "extreme":
        s = sums(case["a"], case["b"], case["xy"], prm["win"])
        kind, other = case["name"].split("-")[1:3]
        if prm["win"] == 31:
            big = np.maximum(s[:, 0], s[:, 2])
            assert (big > 2.0 ** 32).all(), "%s: A11 / A22 %g" % (case["name"], big.min())
            if other == "shift":
                assert (np.maximum(np.abs(s[:, 3]), np.abs(s[:, 4])) > 2.0 ** 31).all(), "%s: |b| %g" % (case["name"], np.abs(s[:, 3:]).max(axis=1).min())
            else:                   # half a period away the products cancel but for one window column
                assert (np.abs(s[:, 3:]) <= 31 * 8160 * 4080.0 * 1.000001).all()
            if kind == "d":
                assert (np.abs(s[:, 1]) > 2.0 ** 32).all()
        return dict(A11=float(s[:, 0].max()), A12=float(np.abs(s[:, 1]).max()), A22=float(s[:, 2].max()), b=float(np.abs(s[:, 3:]).max()))
    return {}


# ---- what a result is held to ----------------------------------------------------------------------------------------------------------
def hold(case, got, mut=None):
    """the (xy_out, status, iters) of the case's call against the definition (or ONE mutant of it) -> (refused, figures).
    refused = the reasons the result is not what the definition allows (empty = held)."""
    k, prm = case["kind"], case["prm"]
    why = []
    if k == "step":
        r = D.check_step(case["a"], case["b"], case["xy"], got, prm["win"], mut=mut)
        if r["undecidable"] > UNDECIDABLE_CAP:
            why.append("undecidable share %.3f" % r["undecidable"])
        if r["violations"]:
            why.append("%d of %d steps outside their bound, worst %.2f of it" % (r["violations"], r["n"], r["worst_ratio"]))
        return why, r
    r = D.check(case["a"], case["b"], case["xy"], got, TAU, mut=mut, **prm)
    if r["nonfinite_bad"]:
        why.append("%d non-finite inputs mishandled" % r["nonfinite_bad"])
    if r["status_diff"]:
        why.append("%d status bytes differ where the definition decides" % r["status_diff"])
    if k == "extreme":              # a binary texture of period 4 is no band-limited image: where a track ends hangs on which iterate trips the
        return why, r               # 0.01 oscillation test, and quantisation moves that.  Positions are held by the step-extreme cases instead.
    tr = r["decided"] & (r["status"] == 0)
    far = int((tr & ~(r["dist"] <= TAU * 1.0001 + 1e-4)).sum())          # (+ float32: half an ulp of a coordinate below 1024 is under 1e-4)
    r["share_beyond"] = far / float(max(int(tr.sum()), 1))
    corridor = "corridor" in case["name"] or k == "fb" or case["name"].startswith("track-osc")
    if far > (BEYOND_CAP * tr.sum() if corridor else 0):
        why.append("%d of %d tracked points beyond tau, worst %.4f px" % (far, tr.sum(), np.nanmax(np.where(tr, r["dist"], 0))))
    if k == "fb":
        i = case["pick"]
        want = 0 if case["name"].endswith("above") else D.ST_FB
        if not r["decided"][i] or r["status"][i] != want:
            why.append("the picked point: status %d decided %s, the case is built for %d" % (r["status"][i], r["decided"][i], want))
    if k == "eig" and not case["name"].endswith("zero"):
        want = D.ST_EIG if ("above" in case["name"]) else 0
        if case["name"].endswith("between"):
            if not (r["decided"].all() and len(set(r["status"].tolist())) == 2):
                why.append("min_eig between the points' values must split them: %s" % r["status"])
        elif not (r["decided"].all() and (r["status"] == want).all()):
            why.append("status %s decided %s, the case is built for %d" % (r["status"], r["decided"], want))
    return why, r
