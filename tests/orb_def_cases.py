"""The cases, the pyramid, the wrong implementations and the symmetry checks that tests/test_orb_def.py (the oracle, CPU) and
tests/test_gpu_orb_definitions.py (csrc/orb.hip) share.  The definitions themselves are tests/orb_def.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_pair as BP                      # noqa: E402
import orb_def as OD                       # noqa: E402

NFEATURES = (4000, 2000, 300, 50, 7)
IMAGES = ("canvas", "noise", "binary", "odd")
MASKS = ("none", "m255", "m1", "empty")
BITS_CAP = 0.35                            # share of descriptor bits the definition may leave undecided, per image
SELECT_CAP = 8                             # candidates the selection rule may leave undecided, per request
MIN_DECIDED_OUT = 10                       # exclusions a request with selection active must let the rule decide


def image(name):
    if name == "canvas":
        return BP.canvas(160, 120, seed=5)
    if name == "noise":
        return np.random.default_rng(1).integers(0, 256, (120, 160)).astype(np.uint8)
    if name == "binary":                   # the canvas binarised by bit 5 of its grey value: every FAST score is 254, so scores tie in
        # droves.  (Binarised by a threshold it keeps 29 keypoints at level 0 -- strict suppression removes every tied neighbour --
        # which is below the 100 the coverage conditions ask for; bit 5 flips more often and keeps 109.)
        return (((BP.canvas(160, 120, seed=5) >> 5) & 1) * 255).astype(np.uint8)
    if name == "odd":                      # 131 x 97: no multiple of any tile, three levels above the 62-pixel rule.  (Seed 4 and not 3: with
        # seed 3 no pixel inside the border has a FAST score of exactly 19, so `>=` for `>` in the segment test changed nothing.)
        return np.random.default_rng(4).integers(0, 256, (97, 131)).astype(np.uint8)
    raise KeyError(name)


def mask(name, shape):
    if name == "none":
        return None
    if name == "empty":
        return np.zeros(shape, np.uint8)
    m = (np.random.default_rng(2).integers(0, 4, shape) > 0).astype(np.uint8)          # three pixels of four pass
    return m * 255 if name == "m255" else m


def build_levels(O, img, m):
    """[(image, mask)] * 8: level 0 the input, level l the oracle's exact linear resize of level l - 1 to the oracle's level
    size; the mask likewise, then zero wherever it fell below 255 (so a {0, 1} mask admits nothing above level 0)."""
    h, w = img.shape
    lv = [(np.ascontiguousarray(img), None if m is None else np.ascontiguousarray(m))]
    for l in range(1, OD.NLEVELS):
        lw, lh = O.orb_level_size(w, h, l)
        pi, pm = lv[-1]
        ml = None
        if pm is not None:
            ml = O.resize_linear_exact(pm, lw, lh)
            ml = np.where(ml > 254, ml, 0).astype(np.uint8)
        lv.append((O.resize_linear_exact(pi, lw, lh), ml))
    return lv


_prepared = {}


def levels_of(O, iname, mname):
    key = (iname, mname)
    if key not in _prepared:
        img = image(iname)
        m = mask(mname, img.shape)
        _prepared[key] = (img, m, OD.prepare(build_levels(O, img, m)))
    return _prepared[key]


# ---- the resize the pyramid is made of, by its definition -------------------------------------------------------------------------
def resize_ref(src, dw, dh):
    """Bilinear resize with pixel centres at half-integers and the border replicated, float64 -> (value, bound).

    bound: an 8-bit implementation rounds each of its two interpolation weights to a multiple of 1/256, so a weight is off by at
    most 1/512.  Along a row that moves the result by at most |p1 - p0| / 512 (e0, e1 for the two rows); between rows the weight
    m is convex, so the row errors contribute at most max(e0, e1), and m's own error at most |T1 - T0| / 512 for the true row
    values T0, T1; rounding to 8 bits adds 0.5 (the products are held exactly until then)."""
    S = np.asarray(src).astype(np.float64)
    sh, sw = S.shape

    def axis(sn, dn):
        f = (np.arange(dn) + 0.5) * (sn / dn) - 0.5
        i = np.floor(f).astype(np.int64)
        t = f - i
        lo, hi = np.clip(i, 0, sn - 1), np.clip(i + 1, 0, sn - 1)
        t = np.where((i < 0) | (i >= sn - 1), 0.0, t)
        lo = np.where(i >= sn - 1, sn - 1, lo)
        return lo, hi, t
    x0, x1, tx = axis(sw, dw)
    y0, y1, ty = axis(sh, dh)
    rows = S[:, x0] * (1 - tx) + S[:, x1] * tx
    erow = np.abs(S[:, x1] - S[:, x0]) * (tx > 0) / 512.0
    T0, T1 = rows[y0], rows[y1]
    val = T0 * (1 - ty[:, None]) + T1 * ty[:, None]
    bound = 0.5 + np.maximum(erow[y0], erow[y1]) + np.abs(T1 - T0) * (ty[:, None] > 0) / 512.0 + 1e-9
    return val, bound


# ---- wrong implementations, one field each ----------------------------------------------------------------------------------------
def model_bits(src, x, y, angle_deg, **turned):
    """Descriptor bits from comparing `src` (any float image of the level) at the rounded turned points."""
    x, y = np.asarray(x, np.int64)[:, None], np.asarray(y, np.int64)[:, None]
    X0, Y0, X1, Y1 = (np.rint(v).astype(np.int64) for v in OD.turn(angle_deg, **turned))
    return src[y + Y0, x + X0] < src[y + Y1, x + X1]


def _rows_of(result):
    octave = np.asarray(result["octave"]).astype(np.int64)
    scale = np.array([OD.level_scale(l) for l in range(OD.NLEVELS)], np.float32)[octave]
    kx = np.rint(result["xy"][:, 0].astype(np.float64) / scale).astype(np.int64)
    ky = np.rint(result["xy"][:, 1].astype(np.float64) / scale).astype(np.int64)
    return octave, kx, ky


def with_set(result, P, sets):
    """The result with the keypoint set replaced by sets[l] = (x, y) per level: rows it already has are kept as they are, new
    ones get the definition's own response, angle and descriptor."""
    octave, kx, ky = _rows_of(result)
    have = {(int(l), int(a), int(b)): i for i, (l, a, b) in enumerate(zip(octave, kx, ky))}
    out = {k: [] for k in ("xy", "size", "angle", "response", "octave", "desc")}
    for l, (x, y) in enumerate(sets):
        if not len(x):
            continue
        order = np.lexsort((x, y))
        x, y = np.asarray(x)[order], np.asarray(y)[order]
        p = P["per"][l]
        s = OD.level_scale(l)
        val, _ = OD.harris(p["img"], x, y)
        ang = OD.centroid_angle(p["img"], x, y).astype(np.float32)
        ang = np.where(ang >= 360, np.float32(0), ang)
        bits, _ = OD.describe_decisions(p["img"], x, y, ang)
        fresh = dict(xy=np.stack([x.astype(np.float32) * s, y.astype(np.float32) * s], 1), size=np.full(len(x), np.float32(31) * s),
                     angle=ang, response=val.astype(np.float32), octave=np.full(len(x), l, np.int32), desc=OD.pack_bits(bits))
        for i, (a, b) in enumerate(zip(x, y)):
            j = have.get((l, int(a), int(b)))
            for k in out:
                out[k].append(np.asarray(result[k])[j] if j is not None else fresh[k][i])
    return {k: (np.array(v, dtype=np.asarray(result[k]).dtype).reshape((-1,) + np.asarray(result[k]).shape[1:]))
            for k, v in out.items()}


def _per_level(result, P, fn):
    """a field rebuilt level by level: fn(level dict, x, y, angle, rows) -> values for those rows"""
    octave, kx, ky = _rows_of(result)
    parts = {}
    for l in range(OD.NLEVELS):
        sel = np.nonzero(octave == l)[0]
        if len(sel):
            parts[l] = (sel, fn(P["per"][l], kx[sel], ky[sel], np.asarray(result["angle"])[sel]))
    return parts


def _replace(result, field, parts):
    out = {k: np.array(v, copy=True) for k, v in result.items()}
    for sel, v in parts.values():
        out[field][sel] = v
    return out


def _angle_from(offsets=None, swap=False):
    def fn(p, x, y, _):
        m10, m01 = OD.moments(p["img"], x, y, offsets)
        if swap:
            m10, m01 = m01, m10
        a = (np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64))) % 360.0).astype(np.float32)
        return np.where(a >= 360, np.float32(0), a)
    return fn


FIELD_MUTANTS = {
    "descriptor, sin negated": ("desc", lambda p, x, y, a: OD.pack_bits(model_bits(p["blurred"][0], x, y, a, negate_sin=True))),
    "descriptor, table rows shifted by one": ("desc", lambda p, x, y, a: OD.pack_bits(model_bits(p["blurred"][0], x, y, a, shift_rows=1))),
    "descriptor from the unblurred level": ("desc", lambda p, x, y, a: OD.pack_bits(model_bits(p["img"].astype(np.float64), x, y, a))),
    "angle from swapped moments": ("angle", _angle_from(swap=True)),
    "angle over the 31 x 31 square": ("angle", _angle_from(OD.square_offsets())),
    "angle over a disc of radius 14": ("angle", _angle_from(OD.disc_offsets(14))),
    "Harris with k = 0.05": ("response", lambda p, x, y, a: OD.harris(p["img"], x, y, k=0.05)[0].astype(np.float32)),
    "Harris over a 5 x 5 block": ("response", lambda p, x, y, a: OD.harris(p["img"], x, y, block=5)[0].astype(np.float32)),
}
SET_MUTANTS = {
    "FAST with arcs of 8": dict(arc=8),
    "FAST with arcs of 10": dict(arc=10),
    "FAST with >= for >": dict(threshold=19),          # `ring >= I(p) + 20` is `ring > I(p) + 19`
    "NMS with >=": dict(strict=False),
    "border 30": dict(border=30),
}


def field_mutant(name, result, P):
    field, fn = FIELD_MUTANTS[name]
    return _replace(result, field, _per_level(result, P, fn))


def identity_rebuild(result, P):
    """with_set on the result's own set: must change nothing (the mutants' scaffolding is not what `check` refuses)"""
    octave, kx, ky = _rows_of(result)
    return with_set(result, P, [(kx[octave == l], ky[octave == l]) for l in range(OD.NLEVELS)])


def set_mutant(name, result, P, levels):
    """the keypoint set a detector with one wrong constant reports when no quota binds"""
    return with_set(result, P, [OD.candidates(img, m, **SET_MUTANTS[name])[:2] for img, m in levels])


def next_rank_mutant(result, P, nfeatures):
    """quota-th replaced by (quota + 1)-th: on every level where the quota binds, the best candidate that was left out joins"""
    octave, kx, ky = _rows_of(result)
    q = OD.quotas(nfeatures)
    sets, added = [], 0
    for l, p in enumerate(P["per"]):
        x, y = kx[octave == l], ky[octave == l]
        if len(p["x"]) > q[l] > 0:
            have = set(zip(x.tolist(), y.tolist()))
            first = np.ones(len(p["x"]), bool)
            if len(first) > 2 * q[l]:
                first = p["score"] >= np.sort(p["score"])[::-1][2 * q[l] - 1]
            out =[i for i in np.argsort(-p["value"], kind="stable") if first[i] and (int(p["x"][i]), int(p["y"][i])) not in have]
            if out:
                x, y = np.append(x, p["x"][out[0]]), np.append(y, p["y"][out[0]])
                added += 1
        sets.append((x, y))
    assert added, "no level of this request has a quota that binds"
    return with_set(result, P, sets)


# ---- symmetries, level 0 only (the fixed-point resize is not symmetric at coefficient ties) -------------------------------------
def _level0(result):
    sel = np.asarray(result["octave"]) == 0
    x = np.rint(result["xy"][sel, 0]).astype(np.int64)
    y = np.rint(result["xy"][sel, 1]).astype(np.int64)
    return x, y, {k: np.asarray(v)[sel] for k, v in result.items()}


def _match(x, y, x2, y2):
    """rows of the second set in the order of the first; both must be the same set"""
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(x2, y2))}
    assert len(at) == len(x2) == len(x), "the sets differ in size: %d and %d" % (len(x), len(x2))
    idx = np.array([at.get((int(a), int(b)), -1) for a, b in zip(x, y)], np.int64)
    assert (idx >= 0).all(), "%d keypoints have no image under the symmetry" % int((idx < 0).sum())
    return idx


def quarter_turn(run, img):
    """run(np.rot90(img)) against run(img): pixel (x, y) goes to (y, W - 1 - x), a direction turns by -90 degrees."""
    W = img.shape[1]
    x, y, a = _level0(run(img))
    x2, y2, b = _level0(run(np.ascontiguousarray(np.rot90(img))))
    idx = _match(y, W - 1 - x, x2, y2)
    assert np.array_equal(a["response"].view(np.uint32), b["response"][idx].view(np.uint32)), "responses differ in some bit"
    da = OD.angle_diff(b["angle"][idx].astype(np.float64), a["angle"].astype(np.float64) - 90.0)
    assert (da <= 1e-3).all(), "angles are not shifted by a quarter turn: worst %.6f deg" % da.max()
    diff = OD.unpack_bits(a["desc"]) != OD.unpack_bits(b["desc"][idx])
    Xa, Xb = OD.turn(a["angle"]), OD.turn(b["angle"][idx])
    tie = np.zeros(diff.shape, bool)
    for v in Xa + Xb:
        tie |= OD.near_half(v)
    assert not (diff & ~tie).any(), "%d descriptor bits differ away from every rounding tie" % int((diff & ~tie).sum())
    return dict(n=len(x), angle=float(da.max()) if len(x) else 0.0, bits_differ=int(diff.sum()))


def mirror(run, img):
    """run(img[:, ::-1]) against run(img): pixel (x, y) goes to (W - 1 - x, y), an angle a to 180 - a."""
    W = img.shape[1]
    x, y, a = _level0(run(img))
    x2, y2, b = _level0(run(np.ascontiguousarray(img[:, ::-1])))
    idx = _match(W - 1 - x, y, x2, y2)
    assert np.array_equal(a["response"].view(np.uint32), b["response"][idx].view(np.uint32)), "responses differ in some bit"
    da = OD.angle_diff(b["angle"][idx].astype(np.float64), 180.0 - a["angle"].astype(np.float64))
    assert (da <= 1e-3).all(), "angles are not mirrored: worst %.6f deg" % da.max()
    return dict(n=len(x), angle=float(da.max()) if len(x) else 0.0)


def hold_request(result, O, iname, mname, nfeatures, what):
    """check + the coverage conditions on the reference that keep these tests from passing on nothing -> figures"""
    img, m, P = levels_of(O, iname, mname)
    f = OD.check(result, img, m, nfeatures, P)
    print(OD.figures_line(what, f))
    if nfeatures == 4000:
        assert f["set_equality"], "precondition: no quota binds at 4000 features (candidates %s, quotas %s)" % (f["candidates"], f["quotas"])
        assert f["n"] == sum(f["candidates"])
    if mname == "empty":
        assert f["n"] == 0
    if nfeatures == 4000 and mname == "none":
        assert f["undecidable_share"] <= BITS_CAP, f["undecidable_share"]
        assert f["per_level"][0] >= 100, f["per_level"]
        assert sum(c > 0 for c in f["per_level"]) >= 2, f["per_level"]
    if f["excess"] > 0:
        assert f["select_undecidable"] <= SELECT_CAP, f["select_undecidable"]
        if f["excess"] >= MIN_DECIDED_OUT:           # (a request that drops fewer candidates than that cannot have as many decided)
            assert f["decided_out"] >= MIN_DECIDED_OUT, f["decided_out"]
    return f
