"""MODE_SGBM_3WAY (mode 2 of vo_set_sgbm) stated on tests/sgbm_def.py: MODE_SGBM with the direction set W, N, E in place of W, NW,
N, NE, E and NOTHING else changed -- the cost volume, eq. 13 with the zero vector outside the band, S = min(L_W + L_N + L_E,
32767), the winner stage and both post filters are DEF's own functions, called here; DEF.MODE_DIRS is not patched.  The N path
runs from the top row to the bottom row of the image as one stripe.  There is no oracle for this mode and no claim of parity
with OpenCV's computeDisparity3WAY (whose stripes depend on the thread count): this definition is the yardstick, and whoever is
compared with it is compared for EQUALITY.

CASES3 are the device cases of tests/sgbm_def_cases.py (gpu, no strip width: strips mean nothing without a diagonal sweep) with
mode 2, one per distinct (scene, shape, seed, parameters); names lose their mode suffix.  The schedule a case must take is VERT /
VERT_RAGGED / UNFUSED by the rule of sgbm_def_cases._case.  The coverage conditions are those of hold_coverage, evaluated on this
definition alone, with two differences that the three-path sums force:
    block7-minD0   seed 0 leaves the left-right check nothing to remove with three paths (0 pixels): seed 1 (4 pixels)
    saturating     "every sum saturated" is not reachable with three paths on that scene (0 pixels at preFilterCap 1, 31 and 63);
                   asked instead: >= 1000 cells whose UNCLAMPED three-path sum exceeds 32767 (3247 at w = 100, h = 24, minD 0,
                   cap 1), so that a sum wrapped in int16 on the device would win the minimum and show"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402

DIRS3 = ("W", "N", "E")
VERT, VERT_RAGGED, UNFUSED = "vert", "vert-ragged", "unfused"


def compute3(L, R, params, info=None, dirs=DIRS3):
    """-> dict(C, S, raw, median, final): every stage of one pair in mode 2.  dirs: another direction set, for the tests that show
    that the cases tell it from the definition.  info receives the winner stage's counts and `over`, the cells whose unclamped
    sum exceeds 32767."""
    h, w = np.asarray(L).shape
    e = DEF.effective(params, w)
    if e.W1 <= 0:
        raw = np.full((h, w), e.invalid, np.int16)
        Cv = S = None
    else:
        Cv = DEF.cost_volume(L, R, params)
        U = sum(DEF.path(Cv, *DEF.DIRS[n], e.P1, e.P2) for n in dirs)
        S = np.minimum(U, DEF.MAX_S)
        raw = DEF.wta(S, e, w, info=info)
        if info is not None:
            info["over"] = int((U > DEF.MAX_S).sum())
    med, fin = DEF.post(raw, e)
    return dict(C=Cv, S=S, raw=raw, median=med, final=fin)


def _name(n):
    for suffix in ("-m0", "-m1"):
        if n.endswith(suffix):
            return n[:-len(suffix)]
    return n


def _cases3():
    out, seen = [], set()
    for c in C.CASES:
        if not c.gpu or c.waves is not None:
            continue
        key = (c.scene, c.w, c.h, c.seed) + tuple(sorted(c.p.items()))
        if key in seen:
            continue
        seen.add(key)
        W1 = DEF.effective(c.p, c.w).W1
        sched = UNFUSED if c.p["uniquenessRatio"] >= 100 else (VERT if W1 % 8 == 0 and W1 >= 16 else VERT_RAGGED)
        name = _name(c.name)
        out.append(c._replace(name=name, mode=2, sched=sched, seed=1 if name == "block7-minD0" else c.seed))
    return out


CASES3 = _cases3()
BY_NAME3 = {c.name: c for c in CASES3}
assert len(BY_NAME3) == len(CASES3)
NAMES3 = [c.name for c in CASES3]

_defs = {}


def definition3(case):
    """the definition's stages of a case and the counts of what each rule decided: computed once, never changed"""
    if case.name not in _defs:
        L, R = C.images(case)
        info = {}
        d = compute3(L, R, case.p, info)
        for a in d.values():
            if a is not None:
                a.setflags(write=False)
        e = DEF.effective(case.p, case.w)
        band = d["final"][:, e.x0:e.x1]
        ok = band >= e.minD * 16
        info.update(share=float(ok.mean()) if ok.size else 0.0, subpixel_share=float(((band[ok] & 15) != 0).mean()) if ok.any() else 0.0)
        if e.window > 0:
            info["speckle"] = int((d["final"] != d["median"]).sum())
        _defs[case.name] = (d, info)
    return _defs[case.name]


def figures3(case):
    i = definition3(case)[1]
    return ("%s: %d x %d, D %d, mode 2, %s: valid %.1f %% of the band, sub-pixel %.1f %% of those; no winner %d, uniqueness %d, "
            "left-right %d, disp2 ties %d, minimum twice apart %d, unclamped sums over 32767 %d, speckle %s"
            % (case.name, case.w, case.h, case.p["numDisparities"], case.sched, 100 * i["share"], 100 * i["subpixel_share"],
               i["no_winner"], i["uniqueness"], i["left_right"], i["disp2_ties"], i["min_twice_apart"], i["over"], i.get("speckle", "off")))


def tie_dependent3(case):
    """pixels of the final result that change when the tie rule of disp2 is turned round"""
    d = definition3(case)[0]
    e = DEF.effective(case.p, case.w)
    return int((DEF.post(DEF.wta(d["S"], e, case.w, mut="disp2_ge"), e)[1] != d["final"]).sum())


def hold_coverage3(case):
    """the scene's conditions (sgbm_def_cases.hold_coverage, with the two differences of the module text), on this definition
    alone -> its figures"""
    i = definition3(case)[1]
    what = figures3(case)
    if case.scene == "layered" and case.p["uniquenessRatio"] < 99 and case.h > 2:
        assert i["share"] >= 0.5, what
        assert i["subpixel_share"] >= 0.05, what
        assert i["uniqueness"] >= 1 and i["left_right"] >= 1, what
    if case.scene == "double":
        if case.p["uniquenessRatio"] >= 100:
            assert i["valid"] >= 0.4 * case.w * case.h, what
        else:
            assert tie_dependent3(case) >= 50, (what, tie_dependent3(case))
    if case.scene.startswith("periodic"):
        assert i["min_twice_apart"] >= 200, what
    if case.scene == "saturating":
        assert i["over"] >= 1000, what
    if case.scene == "speckled":
        assert i["speckle"] >= 20 and i["left_right"] >= 1, what
    return i
