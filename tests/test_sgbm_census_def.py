"""The census cost on the CPU: tests/sgbm_census_def.py against answers written out by hand, its cases' coverage conditions on the
definition alone, and the evidence that a comparison with that definition can fail:

    known answers     the 3 x 3 signatures of a 5 x 4 image as literal sets (clamped borders, one neighbour = centre tie), the Hamming
                      distance of two literal signatures, C of a one-row pair at blockSize 1
    coverage          every case of CASES_CENSUS holds its conditions (hold_coverage_census)
    mutants           each wrong variant (<= for <, zero border, rows not clamped, window transposed, the box sum's two wrong
                      borders, no + P2) changes the final image of at least one case; which cases tell which is printed
    invariance        two strictly increasing grey-level tables on the two images: the census result is identical, BT's is not
    identical images  3 x 3, blockSize 1: d = 0 wins wherever the band allows it
    quality           BT against census 9 x 7 on one SYNTHETIC corridor pair (C1, pair 3, 640 x 480, D = 64, after median3), as it
                      is and with the right image through one fixed gain / offset table: the table of the README

tests/test_gpu_sgbm_census.py holds csrc/sgbm_census.inc to the same definition on the same cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402
import sgbm_census_def as Z        # noqa: E402

IMG = np.array([[5, 3, 8, 1, 4],
                [2, 7, 7, 6, 0],
                [9, 4, 3, 5, 5],
                [1, 6, 2, 8, 7]], np.uint8)
# (x, y) -> the offsets (dx, dy) of its 3 x 3 window whose pixel is strictly darker, coordinates clamped; (1, 1) = 7 has the equal
# neighbour (2, 1) = 7 at (1, 0), which is NOT in its set, and (2, 1) has (1, 1) at (-1, 0), which is not in its set either
SIGNATURES = {
    (0, 0): {(1, -1), (1, 0), (-1, 1), (0, 1)},
    (1, 0): {(-1, 1)},
    (2, 0): {(-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)},
    (3, 0): {(1, 1)},
    (4, 0): {(-1, -1), (-1, 0), (0, 1), (1, 1)},
    (0, 1): set(),
    (1, 1): {(-1, -1), (0, -1), (-1, 0), (0, 1), (1, 1)},
    (2, 1): {(-1, -1), (1, -1), (1, 0), (-1, 1), (0, 1), (1, 1)},
    (3, 1): {(0, -1), (1, -1), (1, 0), (-1, 1), (0, 1), (1, 1)},
    (4, 1): set(),
    (0, 2): {(-1, -1), (0, -1), (1, -1), (1, 0), (-1, 1), (0, 1), (1, 1)},
    (1, 2): {(-1, -1), (1, 0), (-1, 1), (1, 1)},
    (2, 2): {(0, 1)},
    (3, 2): {(1, -1), (-1, 0), (-1, 1)},
    (4, 2): {(0, -1), (1, -1)},
    (0, 3): set(),
    (1, 3): {(0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1)},
    (2, 3): set(),
    (3, 3): {(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1)},
    (4, 3): {(-1, -1), (0, -1), (1, -1)},
}


def test_signatures_of_a_small_image_written_out_by_hand():
    sig = Z.census(IMG, 3, 3)
    assert sig.shape == (4, 5, 8) and len(Z.offsets(9, 7)) == 62
    for (x, y), want in SIGNATURES.items():
        assert Z.signature(sig, 3, 3, x, y) == want, (x, y)
    ge = Z.census(IMG, 3, 3, "ge")
    assert Z.signature(ge, 3, 3, 1, 1) == SIGNATURES[(1, 1)] | {(1, 0)}           # the tie, and no clamped neighbour (none is the centre here)
    assert Z.signature(ge, 3, 3, 0, 1) == {(-1, 0)}                               # the darkest pixel of its window: its own clamped copy alone


def test_hamming_distance_of_two_literal_signatures():
    a, b = SIGNATURES[(2, 1)], SIGNATURES[(3, 1)]
    # differ in (-1, -1) and (0, -1): two comparisons
    offs = Z.offsets(3, 3)
    va, vb = [o in a for o in offs], [o in b for o in offs]
    assert Z.hamming(va, vb) == 2 == len(a ^ b)
    assert Z.hamming(va, va) == 0 and Z.hamming([o in SIGNATURES[(2, 0)] for o in offs], [False] * 8) == 7


def test_cost_volume_of_a_one_row_pair_written_out_by_hand():
    """One row: the rows above and below are the row itself, so of the eight comparisons the three at dx = -1 are one bit (left
    neighbour darker), the three at dx = +1 another, the two at dx = 0 never set: a pixel cost is 3 x (left bits differ) + 3 x
    (right bits differ).
        L = 3 1 4 1 5 9   (left, right) bits: FT FF TT FF TF TF
        R = 1 4 1 5 9 2                       FF TT FF TF TT FF
    D = 2, minD 0: the band is x = 2 .. 5; C[x - 2][k] = P2 + cost(L at x, R at x - k)"""
    L, R = np.array([[3, 1, 4, 1, 5, 9]], np.uint8), np.array([[1, 4, 1, 5, 9, 2]], np.uint8)
    p = dict(minDisparity=0, numDisparities=2, blockSize=1, P1=1, P2=8)
    want = 8 + np.array([[[6, 0], [3, 0], [3, 0], [3, 3]]])
    got = Z.cost_volume(L, R, p, 3, 3)
    assert got.shape == (1, 4, 2) and np.array_equal(got, want), got.tolist()
    assert np.array_equal(Z.cost_volume(L, R, p, 3, 3, "no_p2"), want - 8)


def test_the_cases_are_the_device_cases_with_their_modes_windows_and_twins():
    base = [c for c in Z.CASES_CENSUS if not c.name.endswith("-m2") and c.name not in ("tiles-200x40", "thin-48x16")]
    def key(c, seed):
        return (c.scene, c.w, c.h, seed) + tuple(sorted((k, v) for k, v in c.p.items() if k not in ("P1", "P2")))
    want = {key(c, c.seed) for c in C.CASES if c.gpu and c.waves is None}
    assert {key(c, C.BY_NAME[c.name].seed) for c in base} == want                 # (the seeds this cost moves: sgbm_census_def.SEEDS)
    assert all(c.seed == Z.SEEDS.get(c.name, C.BY_NAME[c.name].seed) for c in base)
    assert len(base) == len(want) == 37 and len(Z.CASES_CENSUS) == 42
    for c in base:
        assert c.mode == C.BY_NAME[c.name].mode
        bs = c.p["blockSize"]
        assert (c.p["P1"], c.p["P2"]) == ((1000, 8000) if c.scene == "saturating" else (2 * bs * bs, 8 * bs * bs))
        if c.name.startswith(("regs-", "block")):
            assert (c.cw, c.ch) == (9, 7)
    assert {(c.cw, c.ch) for c in Z.CASES_CENSUS} == {(3, 3), (5, 5), (7, 7), (9, 7), (9, 3), (3, 7)}
    assert sorted(c.name for c in Z.CASES_CENSUS if c.mode == 2) == ["block5-minD3-m2", "pair-79x17-m2", "we2-96x21-m2"]
    t, n = Z.BY_NAME["tiles-200x40"], Z.BY_NAME["thin-48x16"]
    assert (t.w, t.h, t.p["numDisparities"], t.cw, t.ch, n.w, n.h, n.cw, n.ch) == (200, 40, 32, 9, 7, 48, 16, 9, 7)
    scheds = {s: sum(c.sched == s for c in Z.CASES_CENSUS) for s in (C.DIAG, C.RAGGED, C.UNFUSED, Z.T3.VERT, Z.T3.VERT_RAGGED)}
    print("schedules: %s" % scheds)
    assert all(v >= 1 for v in scheds.values())
    assert {(c.p["numDisparities"] + 31) // 32 for c in Z.CASES_CENSUS} == set(range(1, 9))
    assert {c.p["blockSize"] for c in Z.CASES_CENSUS} >= {1, 3, 5, 7, 9, 11}


@pytest.mark.parametrize("name", Z.NAMES)
def test_every_case_holds_its_conditions(name):
    c = Z.BY_NAME[name]
    i = Z.hold_coverage_census(c)
    d = Z.definition(c)[0]
    print(Z.figures(c))
    e = DEF.effective(c.p, c.w)
    assert d["S"].max() <= DEF.MAX_S and d["S"].min() >= 0
    assert e.P2 <= d["C"].min() and i["cmax"] <= (2 * e.r + 1) ** 2 * (c.cw * c.ch - 1)


def test_every_mutant_is_told_from_the_definition():
    told = {m: [] for m in Z.MUTANTS}
    for c in Z.CASES_CENSUS:
        if c.p["numDisparities"] > 64:
            continue                                                    # (the wide ranges add time and no new geometry)
        L, R = Z.images(c)
        want = Z.definition(c)[0]["final"]
        for m in Z.MUTANTS:
            if (Z.compute_census(L, R, c.p, c.mode, c.cw, c.ch, mut=m)["final"] != want).any():
                told[m].append(c.name)
    for m in Z.MUTANTS:
        print("%s: told by %d cases: %s" % (m, len(told[m]), ", ".join(told[m])))
    assert all(told[m] for m in Z.MUTANTS), {m: len(v) for m, v in told.items()}


def test_a_square_window_does_not_tell_a_transposed_one():
    """... so the transposed variant has to be told by the 9 x 7, 9 x 3 and 3 x 7 cases, and is"""
    c = Z.BY_NAME["we2-96x21-m0"]
    assert c.cw == c.ch
    L, R = Z.images(c)
    assert np.array_equal(Z.compute_census(L, R, c.p, c.mode, c.cw, c.ch, mut="transposed")["final"], Z.definition(c)[0]["final"])


def test_monotone_grey_level_tables_change_nothing_under_census_and_something_under_bt():
    (L, R), (L2, R2) = Z.invariance_pairs()
    assert not np.array_equal(L, L2) and not np.array_equal(R, R2)
    p_bt = C.params(64)
    p = Z.census_params(p_bt, "layered")
    for mode in (0, 2):
        a, b = Z.compute_census(L, R, p, mode, 9, 7), Z.compute_census(L2, R2, p, mode, 9, 7)
        assert np.array_equal(a["C"], b["C"]) and np.array_equal(a["final"], b["final"])
        e = DEF.effective(p, 96)
        assert (a["final"][:, e.x0:e.x1] >= 0).mean() > 0.5
    a, b = DEF.compute(L, R, p_bt)["final"], DEF.compute(L2, R2, p_bt)["final"]
    print("two monotone tables: census 9 x 7 identical; BT differs in %d of %d pixels" % (int((a != b).sum()), a.size))
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("minD", [0, -3])
def test_identical_images_give_disparity_zero(minD):
    img = np.random.default_rng(7).integers(0, 256, (20, 64)).astype(np.uint8)
    p = C.params(16, minD, bs=1, P1=2, P2=8)
    for mode in (0, 1, 2):
        d = Z.compute_census(img, img, p, mode, 3, 3)
        e = DEF.effective(p, 64)
        assert d["C"][:, :, -minD].max() == e.P2                        # d = 0 costs nothing anywhere
        # (minD 0: d = 0 is the end of the range and takes no sub-pixel step; minD -3: it is inside, and the parabola through its
        # two unequal neighbours moves the result by less than half a pixel)
        band = d["final"][:, e.x0:e.x1]
        assert (band == 0).all() if minD == 0 else ((np.abs(band) < 8).all() and (band == 0).mean() > 0.5), mode
        assert (d["final"][:, :e.x0] == e.invalid).all() and (d["final"][:, e.x1:] == e.invalid).all()


def test_quality_on_one_synthetic_corridor_pair():
    """The table of the README: this project's own definitions on ONE SYNTHETIC pair, not real footage.  The right image's table
    is gain 0.7, offset + 40 (rounded, so a few neighbouring grey levels merge: not strictly increasing, and the census rows may
    differ a little)."""
    from openvo_amd.synth import Corridor
    co = Corridor("C1")
    L, R = co.pair(3)
    table = np.clip(np.rint(np.arange(256) * 0.7 + 40), 0, 255).astype(np.uint8)
    R2 = table[R]
    p_bt = dict(co.sgbm_params(), speckleWindowSize=0)
    p_ce = dict(co.sgbm_params(cost=1), speckleWindowSize=0)
    assert L.shape == (480, 640) and p_bt["numDisparities"] == 64 and (p_ce["P1"], p_ce["P2"], p_ce["censusWidth"], p_ce["censusHeight"]) == (50, 200, 9, 7)
    e = DEF.effective(p_bt, co.w)
    rows = {}
    for what, right in (("as rendered", R), ("right image x 0.7 + 40", R2)):
        for cost in ("BT", "census 9 x 7"):
            info = {}
            if cost == "BT":
                Cv, pe = DEF.cost_volume(L, right, p_bt), e
            else:
                Cv, pe = Z.cost_volume(L, right, p_ce, 9, 7), DEF.effective(p_ce, co.w)
            S = DEF.summed(Cv, 0, pe.P1, pe.P2)
            del Cv
            med = DEF.median3(DEF.wta(S, pe, co.w, info=info))[:, e.x0:e.x1]
            del S
            rows[(cost, what)] = (med, med >= 0, info)
    ref, ref_ok = rows[("BT", "as rendered")][:2]
    print("cost | right image | valid share of the band | uniqueness rejects | left-right rejects | valid in both (this, BT as rendered) | of those, > 1 px off BT as rendered")
    off = {}
    for key in (("BT", "as rendered"), ("census 9 x 7", "as rendered"), ("BT", "right image x 0.7 + 40"), ("census 9 x 7", "right image x 0.7 + 40")):
        med, ok, info = rows[key]
        both = ok & ref_ok
        off[key] = float((np.abs(med[both].astype(np.int64) - ref[both]) > 16).mean())
        print("%s | %s | %.3f | %d | %d | %.3f | %.2f %%" % (key[0], key[1], ok.mean(), info["uniqueness"], info["left_right"], both.mean(), 100 * off[key]))
    shares = {k: float(v[1].mean()) for k, v in rows.items()}
    moved = {c: abs(shares[(c, "right image x 0.7 + 40")] - shares[(c, "as rendered")]) for c in ("BT", "census 9 x 7")}
    print("the table moves the valid share by %.4f under BT and by %.4f under census: %s"
          % (moved["BT"], moved["census 9 x 7"], "census shows no advantage on this pair" if moved["census 9 x 7"] >= moved["BT"] and
             shares[("census 9 x 7", "right image x 0.7 + 40")] <= shares[("BT", "right image x 0.7 + 40")] else "census holds up better on this pair"))
    assert all(s > 0.5 for s in shares.values()), shares
