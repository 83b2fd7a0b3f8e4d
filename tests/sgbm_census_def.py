"""The census cost of the SGBM stage (vo_set_sgbm_cost: VO_SGBM_COST_CENSUS) stated on tests/sgbm_def.py in plain numpy (int64):
a census signature per pixel, the Hamming distance of two signatures as the pixel cost, and from there on DEF's own stages.  There
is no oracle for this cost and OpenCV has no counterpart: this definition is the yardstick, and whoever is compared with it is
compared for EQUALITY.  Nothing of DEF is patched; nothing of oracle/ or openvo_amd/ is imported.

    signature   of pixel (x, y) for a window cw x ch (cw in 3, 5, 7, 9; ch in 3, 5, 7: at most 62 comparisons): the SET of offsets
                (dx, dy) != (0, 0), |dx| <= cw // 2, |dy| <= ch // 2, with I(x + dx, y + dy) < I(x, y) (strict).  Coordinates
                outside the image are clamped (rows and columns replicated).  Bit positions are no part of it: only the number of
                comparisons in which two signatures differ is observable.
    pixel cost  c(y, x, k) = |sig_L(x, y) symmetric difference sig_R(x - (minD + k), y)| at the left columns of DEF.effective's
                computed band, where x - d never leaves the image
    block cost  C = P2 + the (2 r + 1)^2 box sum of the pixel cost, r = blockSize // 2, indices clamped to the band and the image
                rows exactly as DEF.cost_volume clamps them (the lines are restated below); blockSize 1 is the bare Hamming
                cost.  preFilterCap means nothing to this cost.
    the rest    DEF.path / DEF.summed (modes 0 and 1), sgbm_3way_def's direction set (mode 2), DEF.wta, DEF.post

CASES_CENSUS are the device cases of tests/sgbm_def_cases.py (gpu, no strip width), one per distinct (scene, shape, seed,
parameters), each in its own mode and under its own name, with P1 = 2 bs^2 and P2 = 8 bs^2 (sgbm_def_cases.params' rule divided by
4: a Hamming cost is at most 62 where a BT cost reaches some 250) -- the `saturating` cases keep their own P1 1000 / P2 8000.  The
windows 3x3, 5x5, 7x7, 9x7, 9x3 and 3x7 are dealt round over the cases in their order; every regs-*, block* and saturating case takes 9x7.
Mode 2 twins: we2-96x21-m2, pair-79x17-m2, block5-minD3-m2.  Two shapes of their own, because the signature kernel is tiled:
tiles-200x40 (D 32, 9x7: more than one tile each way) and thin-48x16 (D 16, 9x7: 16 rows, the halo of three rows and four columns
meets the clamp on every side).  The schedule a case must take follows sgbm_def_cases._case (modes 0, 1) / sgbm_3way_def._cases3
(mode 2), unchanged.

Coverage (hold_coverage_census), on this definition alone: the scene's conditions of sgbm_def_cases.hold_coverage, and for every
case >= 1 pixel whose signature differs from the "ge" variant's (a neighbour equal to the centre exists) and >= 1 pixel whose
signature differs from the "zero_border" variant's in a border column and one in a border row (clamping acts both ways).  What this
cost cannot reach, with what is asked instead (figures from this file, printed by tests/test_sgbm_census_def.py):
%s"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402
import sgbm_3way_def as T3         # noqa: E402

COST_BT, COST_CENSUS = 0, 1
WIDTHS, HEIGHTS = (3, 5, 7, 9), (3, 5, 7)
MUTANTS = ("ge", "zero_border", "no_row_clamp", "transposed", "box_zero_pad", "box_image_clamp", "no_p2")


def offsets(cw, ch):
    """the comparisons of a cw x ch window as (dx, dy), in the order of the last axis of census()"""
    return [(dx, dy) for dy in range(-(ch // 2), ch // 2 + 1) for dx in range(-(cw // 2), cw // 2 + 1) if (dx, dy) != (0, 0)]


def census(img, cw, ch, mut=None):
    """(H, W, n) bool: per pixel and offset of offsets(cw, ch) whether the neighbour is darker than the centre"""
    assert cw in WIDTHS and ch in HEIGHTS
    if mut == "transposed":
        cw, ch = ch, cw
    I = np.asarray(img).astype(np.int64)
    h, w = I.shape
    rx, ry = cw // 2, ch // 2
    if mut == "zero_border":
        P = np.pad(I, ((ry, ry), (rx, rx)), mode="constant")
    elif mut == "no_row_clamp":
        P = np.pad(np.pad(I, ((0, 0), (rx, rx)), mode="edge"), ((ry, ry), (0, 0)), mode="constant")
    else:
        P = np.pad(I, ((ry, ry), (rx, rx)), mode="edge")
    out = []
    for dx, dy in offsets(cw, ch):
        nb = P[ry + dy:ry + dy + h, rx + dx:rx + dx + w]
        out.append(nb <= I if mut == "ge" else nb < I)
    return np.stack(out, axis=-1)


def signature(sig, cw, ch, x, y):
    """the signature of one pixel as the set of its offsets"""
    return {o for o, b in zip(offsets(cw, ch), sig[y, x]) if b}


def hamming(a, b):
    return int((np.asarray(a, bool) != np.asarray(b, bool)).sum())


def pixel_cost(L, R, e, xa, xb, cw, ch, mut=None):
    """(H, xb - xa, D): the Hamming distance of the two signatures at left columns [xa, xb).  Inside the computed band x - d never
    leaves the image; the clip below only acts for the box_image_clamp variant."""
    h, w = np.asarray(L).shape
    sl, sr = census(L, cw, ch, mut), census(R, cw, ch, mut)
    out = np.zeros((h, xb - xa, e.D), np.int64)
    xs = np.arange(xa, xb)
    for k in range(e.D):
        xr = xs - (e.minD + k)
        if xa == e.x0 and xb == e.x1:
            assert xr.min() >= 0 and xr.max() < w
        xr = np.clip(xr, 0, w - 1)
        out[:, :, k] = (sl[:, xs] != sr[:, xr]).sum(axis=2)
    return out


def cost_volume(L, R, params, cw, ch, mut=None):
    """C (H, W1, D) = P2 + the (2r + 1)^2 box sum of the pixel cost, indices clamped to the computed band and the image rows"""
    h, w = np.asarray(L).shape
    e = DEF.effective(params, w)
    r = e.r
    if mut == "box_image_clamp":
        xa, xb = max(e.x0 - r, 0), min(e.x1 + r, w)
        pix = pixel_cost(L, R, e, xa, xb, cw, ch, mut)
        pix = np.pad(pix, ((r, r), (r - (e.x0 - xa), r - (xb - e.x1)), (0, 0)), mode="edge")
    else:
        pix = pixel_cost(L, R, e, e.x0, e.x1, cw, ch, mut)
        pix = np.pad(pix, ((r, r), (r, r), (0, 0)), mode="constant" if mut == "box_zero_pad" else "edge")
    rows = sum(pix[k:k + h] for k in range(2 * r + 1))
    return sum(rows[:, k:k + e.W1] for k in range(2 * r + 1)) + (0 if mut == "no_p2" else e.P2)


def compute_census(L, R, params, mode, cw, ch, info=None, mut=None):
    """-> dict(C, S, raw, median, final): every stage of one pair under the census cost.  info receives the winner stage's counts
    and `over`, the cells whose unclamped sum exceeds 32767."""
    h, w = np.asarray(L).shape
    e = DEF.effective(params, w)
    if e.W1 <= 0:
        raw = np.full((h, w), e.invalid, np.int16)
        Cv = S = None
    else:
        Cv = cost_volume(L, R, params, cw, ch, mut)
        if mode == 2:
            U = sum(DEF.path(Cv, *DEF.DIRS[n], e.P1, e.P2) for n in T3.DIRS3)
        else:
            U = sum(DEF.path(Cv, *DEF.DIRS[n], e.P1, e.P2) for n in DEF.MODE_DIRS[mode])
        S = np.minimum(U, DEF.MAX_S)
        raw = DEF.wta(S, e, w, info=info)
        if info is not None:
            info["over"] = int((U > DEF.MAX_S).sum())
    med, fin = DEF.post(raw, e)
    return dict(C=Cv, S=S, raw=raw, median=med, final=fin)


def invariance_pairs(seed=0):
    """((L, R), (L', R')): a layered pair (96 x 21, D 64) squeezed into the grey levels 64 .. 191, and the same pair with each image
    passed through a strictly increasing table of its own, 64 .. 191 -> 0 .. 255 in random steps of 1 or 2: the order of any two
    grey levels of one image is the same before and after, so every census signature is, and with it everything behind them"""
    L, R = C.layered(96, 21, 64, 0, seed)
    L, R = (64 + L // 2).astype(np.uint8), (64 + R // 2).astype(np.uint8)
    rng = np.random.default_rng([5, seed])
    out = []
    for img in (L, R):
        table = np.zeros(256, np.int64)
        table[64:192] = np.concatenate([[int(rng.integers(0, 2))], rng.integers(1, 3, 127)]).cumsum()
        assert (np.diff(table[64:192]) >= 1).all() and table[191] <= 255 and img.min() >= 64 and img.max() <= 191
        out.append(table[img].astype(np.uint8))
    return (np.ascontiguousarray(L), np.ascontiguousarray(R)), tuple(np.ascontiguousarray(a) for a in out)


CensusCase = collections.namedtuple("CensusCase", "name scene w h p mode sched gpu seed cw ch")
SPREAD = ((3, 3), (5, 5), (7, 7), (9, 7), (9, 3), (3, 7))
# cases whose seed the census cost forces away from sgbm_def_cases' (see EXCEPTIONS)
SEEDS = {"we-40x17": 1, "regs-D192-h16": 1, "regs-D224-h16": 2, "regs-D256-h16": 6, "rows-96x16": 1, "pair-79x17-m2": 6}


def census_params(p, scene):
    """sgbm_def_cases.params' P1 / P2 rule divided by 4; the saturating scene keeps its own"""
    q = dict(p)
    if scene != "saturating":
        bs = q["blockSize"]
        q["P1"], q["P2"] = 2 * bs * bs, 8 * bs * bs
    return q


def _sched(p, w, mode):
    W1 = DEF.effective(p, w).W1
    even = W1 % 8 == 0 and W1 >= 16
    if p["uniquenessRatio"] >= 100:
        return C.UNFUSED
    if mode == 2:
        return T3.VERT if even else T3.VERT_RAGGED
    return C.DIAG if even else C.RAGGED


def _cases():
    out, seen, k = [], set(), 0
    for c in C.CASES:
        if not c.gpu or c.waves is not None:
            continue
        key = (c.scene, c.w, c.h, c.seed) + tuple(sorted(c.p.items()))
        if key in seen:
            continue
        seen.add(key)
        if c.name.startswith("regs-") or c.name.startswith("block") or c.scene == "saturating":
            win = (9, 7)
        else:
            win = SPREAD[k % len(SPREAD)]
            k += 1
        p = census_params(c.p, c.scene)
        out.append(CensusCase(c.name, c.scene, c.w, c.h, p, c.mode, _sched(p, c.w, c.mode), True, SEEDS.get(c.name, c.seed), *win))
    for name in ("we2-96x21-m0", "pair-79x17", "block5-minD3"):
        c = next(x for x in out if x.name == name)
        n2 = T3._name(name) + "-m2"
        out.append(c._replace(name=n2, mode=2, sched=_sched(c.p, c.w, 2), seed=SEEDS.get(n2, c.seed)))
    p = census_params(C.params(32), "layered")
    out.append(CensusCase("tiles-200x40", "layered", 200, 40, p, 0, _sched(p, 200, 0), True, SEEDS.get("tiles-200x40", 0), 9, 7))
    p = census_params(C.params(16), "layered")
    out.append(CensusCase("thin-48x16", "layered", 48, 16, p, 0, _sched(p, 48, 0), True, SEEDS.get("thin-48x16", 0), 9, 7))
    return out


CASES_CENSUS = _cases()
BY_NAME = {c.name: c for c in CASES_CENSUS}
assert len(BY_NAME) == len(CASES_CENSUS)
NAMES = [c.name for c in CASES_CENSUS]
assert {(c.cw, c.ch) for c in CASES_CENSUS} >= set(SPREAD)

_defs = {}


def images(case):
    return C.images(C.Case(case.name, case.scene, case.w, case.h, case.p, case.mode, case.sched, None, True, case.seed))


def definition(case):
    """the definition's stages of a case and the counts of what each rule decided: computed once, never changed"""
    if case.name not in _defs:
        L, R = images(case)
        info = {}
        d = compute_census(L, R, case.p, case.mode, case.cw, case.ch, info)
        for a in d.values():
            if a is not None:
                a.setflags(write=False)
        e = DEF.effective(case.p, case.w)
        band = d["final"][:, e.x0:e.x1]
        ok = band >= e.minD * 16
        info.update(share=float(ok.mean()) if ok.size else 0.0, subpixel_share=float(((band[ok] & 15) != 0).mean()) if ok.any() else 0.0)
        if e.window > 0:
            info["speckle"] = int((d["final"] != d["median"]).sum())
        ties = edge_c = edge_r = 0
        for img in (L, R):
            s = census(img, case.cw, case.ch)
            ties += int((s != census(img, case.cw, case.ch, "ge")).any(axis=2).sum())
            z = (s != census(img, case.cw, case.ch, "zero_border")).any(axis=2)
            edge_c += int(z[:, 0].sum() + z[:, -1].sum())
            edge_r += int(z[0].sum() + z[-1].sum())
        info.update(ties=ties, clamp_cols=edge_c, clamp_rows=edge_r, cmax=int(d["C"].max()) - e.P2)
        _defs[case.name] = (d, info)
    return _defs[case.name]


def figures(case):
    i = definition(case)[1]
    return ("%s: %d x %d, D %d, mode %d, census %d x %d, %s: valid %.1f %% of the band, sub-pixel %.1f %% of those; no winner %d, "
            "uniqueness %d, left-right %d, disp2 ties %d, minimum twice apart %d, sums over 32767 %d, speckle %s; pixels with a "
            "neighbour = centre %d, border pixels the clamp decides: columns %d, rows %d; largest block cost %d"
            % (case.name, case.w, case.h, case.p["numDisparities"], case.mode, case.cw, case.ch, case.sched, 100 * i["share"],
               100 * i["subpixel_share"], i["no_winner"], i["uniqueness"], i["left_right"], i["disp2_ties"], i["min_twice_apart"],
               i["over"], i.get("speckle", "off"), i["ties"], i["clamp_cols"], i["clamp_rows"], i["cmax"]))


def tie_dependent(case):
    """pixels of the final result that change when the tie rule of disp2 is turned round"""
    d = definition(case)[0]
    e = DEF.effective(case.p, case.w)
    return int((DEF.post(DEF.wta(d["S"], e, case.w, mut="disp2_ge"), e)[1] != d["final"]).sum())


EXCEPTIONS = """\
    left-right check   the seed of sgbm_def_cases leaves it nothing to remove (0 pixels) on six cases; the first seed that does:
                       we-40x17 1 (2 pixels), regs-D192-h16 1 (1), regs-D224-h16 2 (1), regs-D256-h16 6 (2), rows-96x16 1 (16),
                       pair-79x17-m2 6 (2)
    saturating         takes 9x7, the window with the largest costs (3x7 and 9x3 leave 39 and 535 cells over 32767, 3x3 none).
                       "every sum saturated" is reached by 90 pixels of saturating-minD-16-m1 (blocks of 11 x 11 Hamming costs stay
                       below 7502 where BT costs reach 23111), not by 100: asked instead, of both cases >= 1000 cells whose
                       UNCLAMPED sum exceeds 32767 (8564 in mode 0, 21714 in mode 1), so that a sum wrapped in int16 on the device
                       would win the minimum and show, and in mode 1 >= 50 pixels with every sum saturated and >= 100 without"""


def hold_coverage_census(case):
    """the scene's conditions (sgbm_def_cases.hold_coverage, with the differences of the module text) and the two of the
    signature, on this definition alone -> its figures"""
    i = definition(case)[1]
    what = figures(case)
    assert i["ties"] >= 1 and i["clamp_cols"] >= 1 and i["clamp_rows"] >= 1, what
    if case.scene == "layered" and case.p["uniquenessRatio"] < 99 and case.h > 2:
        assert i["share"] >= 0.5, what
        assert i["subpixel_share"] >= 0.05, what
        assert i["uniqueness"] >= 1 and i["left_right"] >= 1, what
    if case.scene == "double":
        if case.p["uniquenessRatio"] >= 100:
            assert i["valid"] >= 0.4 * case.w * case.h, what
        else:
            assert tie_dependent(case) >= 50, (what, tie_dependent(case))
    if case.scene.startswith("periodic"):
        assert i["min_twice_apart"] >= 200, what
    if case.scene == "saturating":
        assert i["over"] >= 1000, what
        if case.mode == 1:
            assert i["no_winner"] >= 50 and i["pixels"] - i["no_winner"] >= 100, what
    if case.scene == "speckled":
        assert i["speckle"] >= 20 and i["left_right"] >= 1, what
    return i


__doc__ = __doc__ % EXCEPTIONS
