"""Inputs of the SGBM definition tests, the cases that reach every arm of the dispatcher in csrc/sgbm.hip, and the coverage
conditions -- each evaluated on tests/sgbm_def.py ALONE and asserted (hold_coverage), so that a silent loss of coverage is a
failure.  All images are deterministic from the seeds written here.

Scenes
    layered          smoothed noise with two disparities in alternating row bands, Gaussian noise (sigma 6) on both images.
                     Cases with uniquenessRatio < 99: half of the band valid, 5 % of the valid pixels with a sub-pixel part,
                     the uniqueness test and the left-right check each remove a pixel.  (Not asked of images of one or two
                     rows: 32 or 64 pixels of one disparity give the left-right check nothing to remove.)
    double_visible   the right image is a texture t; the left is t shifted by a = 3 left of column m = 70 and by b = 14 right of
                     it, noise-free: a strip of the right image is matched exactly from two left positions.  Decides the tie
                     rule of disp2 (>= 50 pixels depend on it) and keeps >= 40 % of the image valid at uniquenessRatio 100.
    periodic         both images tiled with period 9 < D, the left tile shifted by 2, with and without a perturbation of the
                     right image of the same period: the minimum of S is attained at several disparities more than 1 apart
                     (>= 200 pixels).  Decides first against last minimum and < against <= in the uniqueness test.
    saturating       black and white 4 x 4 blocks, the right image upside down, white against black at the right end of the band;
                     blockSize 11, P1 1000, P2 8000, preFilterCap 1, ratio 0: in MODE_HH >= 100 pixels have every sum saturated
                     and >= 100 do not.  At minDisparity -16 every pixel of the band's last column is one of them.
    speckled         a pair of tests/group_inputs.py: >= 20 pixels changed by the speckle filter, >= 1 by the left-right check.
A constant pair is no tie case (columns 0 and w - 1 take ftzero: d = 0 is cheaper beside the right border and the E path
carries that along the row) and is not used as one.

Shapes are w x h; at minDisparity 0 the computed band is W1 = w - D wide.  The library takes images of 16 rows and more: the
cases of fewer rows (gpu=False) hold the oracle to the definition on the CPU and the device test asserts that they are
refused; each has a twin of 16 or 17 rows that reaches the same arm on the device."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_inputs          # noqa: E402
import sgbm_def as DEF       # noqa: E402

DIAG, RAGGED, UNFUSED = "diag", "ragged", "unfused"


def params(D, minD=0, bs=5, ur=10, speckle=0, **over):
    p = dict(minDisparity=minD, numDisparities=D, blockSize=bs, P1=8 * bs * bs, P2=32 * bs * bs, disp12MaxDiff=1, preFilterCap=63,
             uniquenessRatio=ur, speckleWindowSize=speckle, speckleRange=2)
    p.update(over)
    return p


def _texture(rng, h, w):
    """noise smoothed by a 2 x 2 box: texture that a 4-bit sub-pixel step can interpolate"""
    n = rng.integers(0, 256, (h + 1, w + 1)).astype(np.int64)
    return ((n[1:, 1:] + n[1:, :-1] + n[:-1, 1:] + n[:-1, :-1]) // 4).astype(np.uint8)


def _noisy(rng, img, sigma):
    return np.clip(np.rint(img + rng.normal(0, sigma, img.shape)), 0, 255).astype(np.uint8)


def layered(w, h, D, minD=0, seed=0):
    rng = np.random.default_rng([1, w, h, D, minD + 64, seed])
    pad = D + abs(minD) + 8
    t = _texture(rng, h, w + 2 * pad)
    da, db = minD + D // 4, minD + D // 4 + max(3, D // 5)
    d = np.where((np.arange(h) // 5) % 2 == 0, da, db)
    L = t[:, pad:pad + w]
    R = np.stack([t[y, pad + d[y]:pad + d[y] + w] for y in range(h)])
    return _noisy(rng, L, 6), _noisy(rng, R, 6)


def double_visible(w=112, h=20, a=3, b=14, m=70, seed=0):
    rng = np.random.default_rng([2, w, h, a, b, m, seed])
    t = _texture(rng, h, w + 2 * b)
    R = t[:, b:b + w]
    L = np.concatenate([t[:, b - a:b - a + m], t[:, m:m + w - m]], axis=1)          # L[x] = R[x - a], x < m; R[x - b] beyond
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def periodic(w, h, period=9, shift=2, perturbed=False, seed=0):
    rng = np.random.default_rng([3, w, h, period, shift, seed])
    tile = _texture(rng, h, period).astype(np.int64)
    reps = w // period + 2
    R = np.tile(tile, (1, reps))[:, :w]
    L = np.tile(np.roll(tile, shift, axis=1), (1, reps))[:, :w]                       # L[x] = R[x - shift] = R[x - shift - k * period]
    if perturbed:
        R = R + np.tile(rng.integers(-6, 7, (h, period)), (1, reps))[:, :w]
    return np.clip(L, 0, 255).astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)


def saturating(w=100, h=24, minD=0, seed=0):
    rng = np.random.default_rng([4, w, h, seed])
    t = np.kron(rng.integers(0, 2, (h // 4 + 1, (w + 8) // 4 + 1)) * 255, np.ones((4, 4), np.int64))[:h, :w + 8].astype(np.uint8)
    L, R = np.ascontiguousarray(t[:, :w]), np.ascontiguousarray(t[::-1, 5:5 + w])
    # white against black at the right end of the band, where the paths that start there (E, NE, SE) would otherwise keep the
    # sums low.  With minDisparity < 0 every sum of the band's LAST column saturates; at minDisparity 0 none can: that column
    # is image column w - 1, ftzero in both images, so d = 0 costs nothing in six of the eleven columns of its block.
    x1 = w + min(minD, 0)
    L[:, x1 - 12:] = 255
    R[:, w - 40:] = 0
    return L, R


SAT = dict(blockSize=11, P1=1000, P2=8000, preFilterCap=1, uniquenessRatio=0, disp12MaxDiff=1000)

Case = collections.namedtuple("Case", "name scene w h p mode sched waves gpu seed")


def _case(name, scene, w, h, p, mode, sched=None, waves=None, seed=0):
    if sched is None:
        W1 = DEF.effective(p, w).W1
        sched = UNFUSED if p["uniquenessRatio"] >= 100 else (DIAG if W1 % 8 == 0 and W1 >= 16 else RAGGED)
    return Case(name, scene, w, h, p, mode, sched, waves, h >= 16, seed)


def _cases():
    c = []
    # W + E by k_sgbm_we2 (W1 % 16 == 0, W1 >= 32): W1 = 32; 21 rows = 6 four-row groups, 19 rows = 5
    for mode in (0, 1):
        c.append(_case("we2-96x21-m%d" % mode, "layered", 96, 21, params(64), mode, DIAG))
    c.append(_case("we2-96x19", "layered", 96, 19, params(64), 0, DIAG))
    for seed in (1, 2):                                  # with we2-96x21-m0 the three members of the sweep group of the device test
        c.append(_case("we2-96x21-s%d" % seed, "layered", 96, 21, params(64), 0, DIAG, seed=seed))
    # W + E by k_sgbm_we (W1 % 8 == 0, W1 >= 16, not the above): W1 = 24, 16, 40
    c.append(_case("we-40x9", "layered", 40, 9, params(16), 0, DIAG))
    c.append(_case("we-40x17", "layered", 40, 17, params(16), 0, DIAG))
    c.append(_case("we-32x17-m1", "layered", 32, 17, params(16), 1, DIAG))
    c.append(_case("we-56x17", "layered", 56, 17, params(16), 0, DIAG))
    # W + E by k_sgbm_pair (otherwise): W1 = 15, 33
    c.append(_case("pair-79x17", "layered", 79, 17, params(64), 0, RAGGED))
    c.append(_case("pair-49x17-m1", "layered", 49, 17, params(16), 1, RAGGED))
    # registers per lane Dp / 32 = 1 .. 8 (D 16, 64, 96, 128 .. 256) and the padded ranges (16, 48, 112) beside the exact ones
    # (32, 64, 96), at w = D + 40: 12 rows as a case of the definition, 16 rows on the device; each in one mode
    for i, D in enumerate((16, 32, 48, 64, 96, 112, 128, 160, 192, 224, 256)):
        c.append(_case("regs-D%d-h12" % D, "layered", D + 40, 12, params(D), i % 2, seed=1 if D == 256 else 0))   # (seed 0 leaves the left-right check nothing at D 256)
        c.append(_case("regs-D%d-h16" % D, "layered", D + 40, 16, params(D), i % 2))
    # the cost sweep's SW = 0 .. 5 (blockSize 1 .. 11), minDisparity -16, -5, 0, 3 spread over them
    for bs, minD in ((1, -16), (3, -5), (5, 3), (7, 0), (9, -16), (11, -5)):
        c.append(_case("block%d-minD%d" % (bs, minD), "layered", 40 + max(minD + 16, 0) - min(minD, 0), 17,    # W1 = 40
                       params(16, minD, bs), bs // 2 % 2))
    c.append(_case("minD3-m1", "layered", 75, 17, params(16, 3), 1))
    # the unfused arm (k_sgbm_paths, k_sgbm_wta, k_lr_median3, k_ccl_*): uniquenessRatio 100, speckle filter on -- and the
    # same pair on the fused arm, where the tie rule of disp2 is decided
    for mode in (0, 1):
        c.append(_case("double-ur100-m%d" % mode, "double", 112, 20, params(32, ur=100, speckle=30), mode, UNFUSED))
        c.append(_case("double-ur10-m%d" % mode, "double", 112, 20, params(32, ur=10, speckle=30), mode, DIAG))
    # periodic: first against last minimum, < against <=
    for k, (pert, ur, mode) in enumerate(((False, 0, 0), (False, 10, 1), (True, 0, 1), (True, 10, 0))):
        c.append(_case("periodic%s-ur%d-m%d" % ("-pert" if pert else "", ur, mode), "periodic-pert" if pert else "periodic", 96, 18,
                       params(32, ur=ur), mode, DIAG))
    # every sum saturated
    for mode in (0, 1):
        c.append(_case("saturating-m%d" % mode, "saturating", 100, 24, params(16, **SAT), mode))
    c.append(_case("saturating-minD-16-m1", "saturating", 116, 24, params(16, -16, **SAT), 1))      # the band's last column too
    # both post filters at work
    c.append(_case("speckled-k1", "speckled", 112, 40, params(32, bs=5, speckle=150, P1=200, P2=800), 0))
    c.append(_case("speckled-k2-m1", "speckled", 112, 40, params(32, bs=5, speckle=150, P1=200, P2=800), 1))
    # strip width (4 * waves columns of the skewed image): the 96 x 21 case is 2 / 2 / 1 strips wide, 160 x 21 is 5 / 3 / 2
    for waves in (7, 11, 15):
        c.append(_case("strip%d-96x21" % waves, "layered", 96, 21, params(64), waves // 4 % 2, DIAG, waves))
        c.append(_case("strip%d-160x21" % waves, "layered", 160, 21, params(64), 1 - waves // 4 % 2, DIAG, waves))
    # fewer rows than a strip is wide; one row; two rows
    c.append(_case("rows-96x1", "layered", 96, 1, params(64), 0, DIAG))
    c.append(_case("rows-96x2", "layered", 96, 2, params(64), 1, DIAG))
    c.append(_case("rows-96x16", "layered", 96, 16, params(64), 1, DIAG))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
GPU_NAMES = [c.name for c in CASES if c.gpu and c.waves is None]
STRIP_NAMES = [c.name for c in CASES if c.waves is not None]
REFUSED_NAMES = [c.name for c in CASES if not c.gpu]
GROUP_NAMES = ["we2-96x21-m0", "we2-96x21-s1", "we2-96x21-s2"]

_pairs, _defs = {}, {}


def images(case):
    key = (case.scene, case.w, case.h, case.p["numDisparities"], case.p["minDisparity"], case.seed)
    if key not in _pairs:
        D, minD = case.p["numDisparities"], case.p["minDisparity"]
        if case.scene == "layered":
            L, R = layered(case.w, case.h, D, minD, case.seed)
        elif case.scene == "double":
            L, R = double_visible(case.w, case.h)
        elif case.scene.startswith("periodic"):
            L, R = periodic(case.w, case.h, perturbed=case.scene.endswith("pert"))
        elif case.scene == "saturating":
            L, R = saturating(case.w, case.h, minD)
        else:
            L, R = group_inputs.pair(case.w, case.h, 1 if "k1" in case.name else 2, D, minD)
        L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
        L.setflags(write=False)
        R.setflags(write=False)
        _pairs[key] = (L, R)
    return _pairs[key]


def definition(case):
    """the definition's stages of a case with the counts of what each rule decided: computed once, never changed"""
    key = (case.scene, case.w, case.h, case.mode, case.seed) + tuple(sorted(case.p.items()))
    if key not in _defs:
        L, R = images(case)
        info = {}
        d = DEF.compute(L, R, case.p, case.mode, info=info)
        for a in d.values():
            if a is not None:
                a.setflags(write=False)
        e = DEF.effective(case.p, case.w)
        band = d["final"][:, e.x0:e.x1]
        ok = band >= e.minD * 16
        info.update(share=float(ok.mean()) if ok.size else 0.0, subpixel_share=float(((band[ok] & 15) != 0).mean()) if ok.any() else 0.0)
        if e.window > 0:
            info["speckle"] = int((d["final"] != d["median"]).sum())
        _defs[key] = (d, info)
    return _defs[key]


def figures(case):
    i = definition(case)[1]
    return ("%s: %d x %d, D %d, mode %d: valid %.1f %% of the band, sub-pixel %.1f %% of those; no winner %d, uniqueness %d, "
            "left-right %d, disp2 ties %d, minimum twice apart %d, speckle %s"
            % (case.name, case.w, case.h, case.p["numDisparities"], case.mode, 100 * i["share"], 100 * i["subpixel_share"],
               i["no_winner"], i["uniqueness"], i["left_right"], i["disp2_ties"], i["min_twice_apart"], i.get("speckle", "off")))


def tie_dependent(case):
    """pixels of the final result that change when the tie rule of disp2 is turned round"""
    L, R = images(case)
    return int((DEF.compute(L, R, case.p, case.mode, mut="disp2_ge")["final"] != definition(case)[0]["final"]).sum())


def hold_coverage(case):
    """the scene's conditions, on the definition alone -> its figures"""
    i = definition(case)[1]
    what = figures(case)
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
    if case.scene == "saturating" and case.mode == 1:
        assert i["no_winner"] >= 100 and i["pixels"] - i["no_winner"] >= 100, what
    if case.scene == "speckled":
        assert i["speckle"] >= 20 and i["left_right"] >= 1, what
    return i
