"""oracle/src/sgbm.c held to tests/sgbm_def.py -- what an SGBM result means, path by path, in whole-volume numpy -- on the CPU,
and the evidence that a comparison with that definition can fail:

    stage by stage    cost volume, raw disparity, median and final result of the oracle equal the definition's on every case of
                      tests/sgbm_def_cases.py (every arm of the dispatcher in csrc/sgbm.hip, five kinds of scene)
    known answers     of the definition's own stages, worked by hand below, no oracle involved
    mutants           sixteen one-field wrong versions of the definition: each differs from it on some case, each planted
                      scene decides what it was planted for; the mutant x case table is printed
    sweep             uniquenessRatio 0 .. 100 on one summed volume changes the result at 20 ratios or more

tests/test_gpu_sgbm_definitions.py holds csrc/sgbm.hip to the same definition on the same cases."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402

# mutants of the winner stage alone run on the definition's S; the others rebuild the volumes
WTA_MUTANTS = ("lr_one_probe", "uniq_gt0", "uniq_le", "disp2_ge", "subpix_no_den", "subpix_floor", "dceil_16", "last_min")
# one of each group of cases that share a pair, parameters and mode (the strip widths and the 12-row twins add nothing here)
MUTANT_CASES = [n for n in C.NAMES if not n.startswith("strip") and not n.endswith("-h12")]
# the scene planted for a mutant must refuse it; every other mutant is refused somewhere
PLANTED = {"disp2_ge": "double-ur10", "uniq_le": "periodic", "last_min": "periodic", "no_clamp": "saturating-m1",
           "dceil_16": "we2-96x21-m", "lr_one_probe": "we2-96x21-m", "subpix_floor": "we2-96x21-m", "subpix_no_den": "we2-96x21-m"}


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_equals_the_definition_stage_by_stage(oracle, name):
    c = C.BY_NAME[name]
    L, R = C.images(c)
    t = time.perf_counter()
    d, _ = C.definition(c)
    dt = time.perf_counter() - t
    C.hold_coverage(c)
    print("%s; %.3f s in the definition" % (C.figures(c), dt))
    Cv = oracle.sgbm_cost_volume(L, R, c.p)
    assert Cv.shape == d["C"].shape and np.array_equal(Cv, d["C"]), ("cost volume", int((Cv != d["C"]).sum()))
    assert d["S"].max() <= DEF.MAX_S and d["S"].min() >= 0
    raw, med, fin = oracle.sgbm_compute(L, R, c.p, c.mode, stages=True)
    for what, a in (("raw", raw), ("median", med), ("final", fin)):
        assert a.dtype == d[what].dtype and np.array_equal(a, d[what]), (what, int((a != d[what]).sum()))


def test_median_and_speckle_forms_equal_the_oracle_on_random_images(oracle):
    rng = np.random.default_rng(5)
    removed = 0
    for k in range(30):
        h, w = rng.integers(3, 24, 2)
        img = (rng.integers(0, 6, (h, w)) * rng.integers(8, 40)).astype(np.int16)
        img[rng.random((h, w)) < 0.25] = -16
        assert np.array_equal(DEF.median3(img), oracle.median3x3_s16(img))
        window, diff = int(rng.integers(1, 12)), int(rng.integers(0, 48))
        got = DEF.speckle(img, -16, window, diff)
        assert np.array_equal(got, oracle.filter_speckles(img, -16, window, diff)), k
        removed += int((got != img).sum())
    print("speckle: %d pixels removed over 30 images" % removed)
    assert removed >= 1000


def test_path_recursion_by_hand():
    """One row, three columns, three disparities, P1 = 1, P2 = 3, C (which carries + P2) =
           x = 0: [5 3 9]     x = 1: [4 8 3]     x = 2: [7 3 6]
    Path from the west.  x = 0 has no predecessor (the zero vector: min = 0, and min(0, 0 + P1, 0 + P2) = 0): L = C - P2
           = [2 0 6], min 0.
    x = 1: d = 0: 4 + min(2, 0 + 1, 0 + 3) - 0 - 3 = 2;   d = 1: 8 + min(0, 2 + 1, 6 + 1, 3) - 3 = 5;
           d = 2: 3 + min(6, 0 + 1, 3) - 3 = 1                                     -> [2 5 1], min 1
    x = 2: d = 0: 7 + min(2, 5 + 1, 1 + 3) - 1 - 3 = 5;   d = 1: 3 + min(5, 2 + 1, 1 + 1, 4) - 4 = 1;
           d = 2: 6 + min(1, 5 + 1, 4) - 4 = 3                                     -> [5 1 3]
    The path from the east is the same recursion on the mirrored row; a vertical path of a one-row image has no predecessor
    anywhere: C - P2."""
    Cv = np.array([[[5, 3, 9], [4, 8, 3], [7, 3, 6]]], np.int64)
    assert DEF.path(Cv, 1, 0, 1, 3).tolist() == [[[2, 0, 6], [2, 5, 1], [5, 1, 3]]]
    assert np.array_equal(DEF.path(Cv, -1, 0, 1, 3), DEF.path(Cv[:, ::-1], 1, 0, 1, 3)[:, ::-1])
    for name in ("NW", "N", "NE", "SW", "S", "SE"):
        assert np.array_equal(DEF.path(Cv, *DEF.DIRS[name], 1, 3), Cv - 3), name
    # the neighbour d + 1 really is read: with P1 on d - 1 alone, x = 1, d = 0 loses its cheapest way (0 + 1): [3 5 1], and
    # x = 2 becomes 7 + min(3, 4) - 4, 3 + min(5, 3 + 1, 4) - 4, 6 + min(1, 5 + 1, 4) - 4
    assert DEF.path(Cv, 1, 0, 1, 3, mut="p1_one_neighbour")[0].tolist() == [[2, 0, 6], [3, 5, 1], [6, 3, 3]]
    S = DEF.summed(Cv, 0, 1, 3)
    assert np.array_equal(S, DEF.path(Cv, 1, 0, 1, 3) + DEF.path(Cv, -1, 0, 1, 3) + 3 * (Cv - 3))
    assert DEF.summed(Cv + 20000, 0, 1, 3).max() == DEF.MAX_S


def test_subpixel_step_by_hand():
    """D = 3, three pixels, no uniqueness margin, no left-right limit; the winner is d = 1 twice and d = 0 once.
        S = [10 4 7]: den = 10 + 7 - 8 = 9,  ((10 - 7) * 16 + 9) / 18 = 57 / 18 = 3      -> 16 + 3 = 19
        S = [5 4 20]: den = 5 + 20 - 8 = 17, ((5 - 20) * 16 + 17) / 34 = -223 / 34 = -6.56: C truncates to -6 (a floor gives
                      -7, the formula without + den gives -240 / 34 -> -7)                -> 16 - 6 = 10
        S = [4 9 9]:  the winner is d = 0, no neighbour on one side: no step              -> 0
    The band of a 6-column image with D = 3 is columns 3 .. 5; the others are (minD - 1) * 16 = -16."""
    e = DEF.effective(dict(minDisparity=0, numDisparities=3, uniquenessRatio=0, disp12MaxDiff=1000), 6)
    assert (e.x0, e.x1, e.W1, e.invalid, e.P1, e.P2, e.r, e.ftzero) == (3, 6, 3, -16, 2, 5, 2, 15)
    S = np.array([[[10, 4, 7], [5, 4, 20], [4, 9, 9]]], np.int64)
    assert DEF.wta(S, e, 6).tolist() == [[-16, -16, -16, 19, 10, 0]]
    assert DEF.wta(S, e, 6, mut="subpix_floor").tolist() == [[-16, -16, -16, 19, 9, 0]]
    assert DEF.wta(S, e, 6, mut="subpix_no_den").tolist() == [[-16, -16, -16, 18, 9, 0]]
    # every sum saturated: no winner, whatever the ratio
    S[0, 2] = DEF.MAX_S
    assert DEF.wta(S, e, 6).tolist() == [[-16, -16, -16, 19, 10, -16]]


def test_effective_parameters():
    e = DEF.effective(dict(minDisparity=-5, numDisparities=16, blockSize=0, P1=0, P2=0, disp12MaxDiff=-1, preFilterCap=40,
                           uniquenessRatio=-1), 100)
    assert (e.P1, e.P2, e.r, e.ur, e.d12, e.ftzero, e.x0, e.x1, e.invalid) == (2, 5, 2, 10, 1, 41, 11, 95, -96)
    assert DEF.effective(dict(minDisparity=3, numDisparities=16, P1=9, P2=4, preFilterCap=1), 50).P2 == 10


def test_vertical_flip_is_a_symmetry_of_eight_paths_and_not_of_five():
    c = C.BY_NAME["we2-96x21-m1"]
    d, _ = C.definition(c)
    e = DEF.effective(c.p, c.w)
    up = np.ascontiguousarray(d["C"][::-1])
    assert np.array_equal(DEF.summed(up, 1, e.P1, e.P2), d["S"][::-1])
    S5 = DEF.summed(d["C"], 0, e.P1, e.P2)
    n = int((DEF.summed(up, 0, e.P1, e.P2) != S5[::-1]).sum())
    print("five paths: %d of %d sums differ under the flip" % (n, S5.size))
    assert n > S5.size // 2


def _mutant_final(c, mut):
    L, R = C.images(c)
    if mut in WTA_MUTANTS:
        e = DEF.effective(c.p, c.w)
        return DEF.post(DEF.wta(C.definition(c)[0]["S"], e, c.w, mut), e)[1]
    return DEF.compute(L, R, c.p, c.mode, mut=mut)["final"]


@pytest.fixture(scope="module")
def table():
    """mutant x case: pixels of the final result that the mutant changes"""
    return {m: {n: int((_mutant_final(C.BY_NAME[n], m) != C.definition(C.BY_NAME[n])[0]["final"]).sum()) for n in MUTANT_CASES}
            for m in DEF.MUTANTS}


def test_every_mutant_is_refused(table):
    print("pixels changed, mutant x case (cases in the order of sgbm_def_cases.CASES):")
    print("%-18s %s" % ("", " ".join("%4d" % i for i in range(len(MUTANT_CASES)))))
    for m in DEF.MUTANTS:
        print("%-18s %s" % (m, " ".join("%4d" % table[m][n] for n in MUTANT_CASES)))
    for i, n in enumerate(MUTANT_CASES):
        print("%4d = %s" % (i, n))
    for m in DEF.MUTANTS:
        caught = [n for n in MUTANT_CASES if table[m][n] > 0]
        print("%-18s refused by %2d of %d cases, at most %d pixels" % (m, len(caught), len(MUTANT_CASES), max(table[m].values())))
        assert caught, m
        if m in PLANTED:
            planted = [n for n in MUTANT_CASES if n.startswith(PLANTED[m])]
            assert planted and all(table[m][n] >= 1 for n in planted), (m, {n: table[m][n] for n in planted})


def test_the_planted_scenes_meet_their_floors(table):
    for n in MUTANT_CASES:
        C.hold_coverage(C.BY_NAME[n])
    for mode in (0, 1):
        assert table["disp2_ge"]["double-ur10-m%d" % mode] >= 50                       # the tie rule of disp2
        L, R = C.images(C.BY_NAME["double-ur100-m%d" % mode])
        c = C.BY_NAME["double-ur100-m%d" % mode]
        assert (C.definition(c)[0]["final"] >= 0).mean() >= 0.4
        assert (DEF.compute(L, R, c.p, mode, mut="uniq_le")["final"] >= 0).sum() == 0   # with <= nothing survives ratio 100
    for n in MUTANT_CASES:
        if n.startswith("periodic"):
            assert table["last_min"][n] >= 200 and table["uniq_le"][n] >= 200, (n, table["last_min"][n], table["uniq_le"][n])
    assert table["no_clamp"]["saturating-m1"] >= 100


def test_uniqueness_ratio_sweep_has_something_to_see():
    c = C.BY_NAME["we2-96x21-m0"]
    e = DEF.effective(c.p, c.w)
    S = C.definition(c)[0]["S"]
    outs = [DEF.wta(S, e._replace(ur=ur), c.w) for ur in range(101)]
    steps = sum(not np.array_equal(outs[k], outs[k + 1]) for k in range(100))
    print("uniquenessRatio 0 .. 100: the raw result changes at %d of 100 steps; valid pixels %d -> %d -> %d"
          % (steps, (outs[0] >= 0).sum(), (outs[50] >= 0).sum(), (outs[100] >= 0).sum()))
    assert steps >= 20
