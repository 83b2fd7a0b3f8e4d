"""oracle/src/orb.c held to ORB's published definitions (tests/orb_def.py), not to itself, and the checker shown to catch errors.

    definitions   known answers of orb_def itself: an isolated bright pixel, the quotas, the disc, the blur kernel, the atan bound
    resize        oracle.resize_linear_exact, which the pyramid levels of every test here come from, against a float64
                  half-pixel-centre bilinear resize, within the bound of its 8-bit weights (orb_def_cases.resize_ref)
    oracle        orb_def.check on 4 images x 4 masks x nfeatures 4000 / 2000 / 300 / 50 / 7 x both blur kernels, with the
                  coverage conditions (orb_def_cases.hold_request) that keep the checker from passing on nothing
    mutants       fourteen wrong implementations of one field each, built in numpy from the oracle's result: each is refused on
                  each image
    symmetries    a quarter turn and a mirror image of the input, level 0

All of it: about 12 s of CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_def as OD                       # noqa: E402
import orb_def_cases as C                  # noqa: E402


# ---- the definitions' own known answers ------------------------------------------------------------------------------------------
def test_fast_score_known_answers():
    img = np.full((40, 40), 50, np.uint8)
    img[20, 20] = 200                       # every ring pixel 150 darker: the test holds up to t = 149
    img[10, 30] = 90
    s = OD.fast_score(img)
    assert s[20, 20] == 149 and s[10, 30] == 39
    img[5, 5] = 69                          # contrast 19: the test holds up to t = 18, no corner at 20
    assert OD.fast_score(img)[5, 5] == 18 and OD.corner_scores(img)[5, 5] == 0
    assert (OD.fast_score(img)[:3] == -1).all() and (OD.fast_score(img)[:, -3:] == -1).all()
    # an arc of exactly 9 brighter pixels is a corner, an arc of 8 is not
    for arc, corner in ((9, True), (8, False)):
        a = np.full((9, 9), 100, np.uint8)
        for dx, dy in OD.RING[:arc]:
            a[4 + dy, 4 + dx] = 160
        assert (OD.corner_scores(a)[4, 4] == 59) == corner
    keep = OD.nms(np.array([[0, 0, 0, 0], [0, 30, 30, 0], [0, 0, 0, 0]]))
    assert not keep.any()                   # two equal neighbours: strict suppression removes both


def test_quotas_disc_kernel_and_atan_bound():
    assert OD.quotas(500) == [109, 90, 75, 63, 52, 44, 36, 31]
    assert sum(OD.quotas(4000)) == 4000 and OD.quotas(0) == [0] * 8
    d = OD.disc_offsets()
    rows = [int((d[:, 1] == v).sum()) for v in range(0, 16)]
    assert rows == [31, 31, 31, 31, 29, 29, 29, 27, 27, 25, 23, 21, 19, 17, 13, 7], rows       # 2 * umax + 1
    turned = {(int(-v), int(u)) for u, v in d}
    assert turned == {(int(u), int(v)) for u, v in d}, "the disc is not symmetric under a quarter turn"
    assert abs(OD.gauss7().sum() - 1) < 1e-15 and OD.PATTERN.shape == (256, 4) and np.abs(OD.PATTERN).max() == 13
    b = OD.atan_poly_bound()
    print("atan polynomial bound: %.6f deg" % b)
    assert 0.005 < b < 0.02


# ---- the resize under every level >= 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("iname", C.IMAGES)
def test_the_pyramid_resize_is_half_pixel_bilinear(oracle, iname):
    img = C.image(iname)
    lv = C.build_levels(oracle, img, C.mask("m255", img.shape))
    worst, widest = 0.0, 0.0
    for l in range(1, OD.NLEVELS):
        for k in (0, 1):                    # image and mask (before the 254 threshold is what the resize returns; rebuild it)
            src = lv[l - 1][k]
            got = oracle.resize_linear_exact(src, lv[l][0].shape[1], lv[l][0].shape[0])
            val, bound = C.resize_ref(src, got.shape[1], got.shape[0])
            share = np.abs(got - val) / bound
            assert (share <= 1).all(), "level %d: %.3f of the bound at %s" % (l, share.max(), np.unravel_index(share.argmax(), share.shape))
            worst, widest = max(worst, float(share.max())), max(widest, float(bound.max()))
    print("%s: worst resize error %.4f of its bound (bound at most %.3f grey levels)" % (iname, worst, widest))


# ---- the oracle against the definitions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur_mode", (0, 1))
@pytest.mark.parametrize("nfeatures", C.NFEATURES)
@pytest.mark.parametrize("mname", C.MASKS)
@pytest.mark.parametrize("iname", C.IMAGES)
def test_the_oracle_meets_the_definitions(oracle, iname, mname, nfeatures, blur_mode):
    img, m, _ = C.levels_of(oracle, iname, mname)
    r = oracle.orb_detect_and_compute(img, m, nfeatures, blur_mode=blur_mode)
    C.hold_request(r, oracle, iname, mname, nfeatures, "%s, mask %s, %d features, blur %d" % (iname, mname, nfeatures, blur_mode))


@pytest.mark.parametrize("mname", ("none", "m255"))
def test_the_oracle_at_2001_features(oracle, mname):
    """the request tests/test_gpu_orb_definitions.py adds for the device's three-launch selection: the reference must stay inside
    the conditions there too"""
    img, m, _ = C.levels_of(oracle, "noise", mname)
    r = oracle.orb_detect_and_compute(img, m, 2001)
    f = C.hold_request(r, oracle, "noise", mname, 2001, "noise, mask %s, 2001 features" % mname)
    assert f["excess"] > 0, f["excess"]


# ---- the checker catches errors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iname", C.IMAGES)
def test_the_mutants_scaffolding_changes_nothing(oracle, iname):
    img, m, P = C.levels_of(oracle, iname, "none")
    r = oracle.orb_detect_and_compute(img, m, 4000)
    same = C.identity_rebuild(r, P)
    assert all(np.array_equal(same[k], r[k]) and same[k].dtype == r[k].dtype for k in r)
    # and the rows the definition itself fills in for a new keypoint pass the checker: a result made of nothing else
    empty = {k: v[:0] for k, v in r.items()}
    octave, kx, ky = C._rows_of(r)
    own = C.with_set(empty, P, [(kx[octave == l], ky[octave == l]) for l in range(OD.NLEVELS)])
    OD.check(own, img, m, 4000, P)


@pytest.mark.parametrize("name", list(C.FIELD_MUTANTS) + list(C.SET_MUTANTS))
@pytest.mark.parametrize("iname", C.IMAGES)
def test_check_refuses_a_wrong_implementation(oracle, iname, name):
    img, m, P = C.levels_of(oracle, iname, "none")
    r = oracle.orb_detect_and_compute(img, m, 4000)
    OD.check(r, img, m, 4000, P)
    bad = C.field_mutant(name, r, P) if name in C.FIELD_MUTANTS else C.set_mutant(name, r, P, C.build_levels(oracle, img, m))
    with pytest.raises(AssertionError) as e:
        OD.check(bad, img, m, 4000, P)
    print("%s, %s: %s" % (iname, name, str(e.value)[:160]))


@pytest.mark.parametrize("nfeatures", (50, 7))
@pytest.mark.parametrize("iname", C.IMAGES)
def test_check_refuses_the_next_rank(oracle, iname, nfeatures):
    """quota-th replaced by (quota + 1)-th"""
    img, m, P = C.levels_of(oracle, iname, "none")
    r = oracle.orb_detect_and_compute(img, m, nfeatures)
    OD.check(r, img, m, nfeatures, P)
    with pytest.raises(AssertionError, match="the selection rule drops"):
        OD.check(C.next_rank_mutant(r, P, nfeatures), img, m, nfeatures, P)


def test_check_refuses_disorder_and_a_wrong_scale(oracle):
    img, m, P = C.levels_of(oracle, "canvas", "none")
    r = oracle.orb_detect_and_compute(img, m, 4000)
    swapped = {k: v.copy() for k, v in r.items()}
    for v in swapped.values():
        v[[0, 1]] = v[[1, 0]]
    with pytest.raises(AssertionError, match="order"):
        OD.check(swapped, img, m, 4000, P)
    for field in ("xy", "size"):
        off = {k: v.copy() for k, v in r.items()}
        sel = off["octave"] == 1
        off[field][sel] = np.nextafter(off[field][sel], np.float32(1e9))
        with pytest.raises(AssertionError, match=field):
            OD.check(off, img, m, 4000, P)


# ---- symmetries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iname", C.IMAGES)
def test_a_quarter_turn_and_a_mirror_image(oracle, iname):
    img = C.image(iname)

    def run(im):
        return oracle.orb_detect_and_compute(im, None, 4000)
    q, mi = C.quarter_turn(run, img), C.mirror(run, img)
    print("%s: quarter turn of %d keypoints: angles within %.2g deg, %d bits differ (all at rounding ties); mirror: angles within %.2g deg"
          % (iname, q["n"], q["angle"], q["bits_differ"], mi["angle"]))
    assert q["n"] >= 100
