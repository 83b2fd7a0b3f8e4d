"""csrc/orb.hip held to what an ORB result MEANS (tests/orb_def.py), not to its restatement oracle/src/orb.c:

    keypoints     every one a FAST-9/16 corner (sixteen brute-force arcs) that survives strict 3x3 suppression, the 31-pixel
                  border and the mask; with no quota binding (4000 features) the set IS the definitional set, level by level --
                  on levels >= 1 that is also the evidence for k_orb_pyramid, whose levels the product does not expose: the
                  levels here are the oracle's resize, itself held to a float64 bilinear resize in tests/test_orb_def.py
    selection     4000 features go through the three selection launches (and 2001, where a quota binds on them), 2000 / 300 / 50 /
                  7 through k_orb_select: whatever the
                  float64 Harris value decides beyond the float32 bound is in or out as retainBest(2 * quota) and
                  retainBest(quota) have it
    fields        response = the Harris measure within its float32 bound, angle = the intensity centroid's direction within the
                  bound of the atan polynomial, descriptor bit j = published comparison j in the patch turned by that angle,
                  wherever the float64 blur decides it; canonical order, xy and size by the level's scale
    slot          upload_mono + orb_slot on the canvas: the slot path's keypoint arrays meet the same checker
    symmetries    a quarter turn and a mirror image of the input, level 0

The cases, the coverage conditions (orb_def_cases.hold_request) and the fourteen wrong implementations that the checker refuses
are those of tests/test_orb_def.py.  Every test prints its figures.  Images are 160 x 120 or smaller: a few launches each; the
numpy checker takes about 4 s of CPU for the whole module (measured with the oracle's results in place of the device's)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_def_cases as C                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from openvo_amd import _native
    c = _native.Context(0, 704, 512, 64, 4000)
    yield c
    c.close()


def _copy(k):
    return {name: np.array(v, copy=True) for name, v in k.items()}


@pytest.mark.parametrize("nfeatures", C.NFEATURES)
@pytest.mark.parametrize("mname", C.MASKS)
@pytest.mark.parametrize("iname", C.IMAGES)
def test_orb_host_meets_the_definitions(ctx, oracle, iname, mname, nfeatures):
    img, m, _ = C.levels_of(oracle, iname, mname)
    r = _copy(ctx.orb_host(img, m, nfeatures))
    C.hold_request(r, oracle, iname, mname, nfeatures, "%s, mask %s, %d features" % (iname, mname, nfeatures))


@pytest.mark.parametrize("mname", ("none", "m255"))
def test_the_three_launch_selection_with_a_binding_quota(ctx, oracle, mname):
    """At 4000 features no quota binds on images this small, so the three selection launches (nfeatures > 2000) select nothing
    there; at 2001 the noise image's level 0 has more candidates than its quota and they do."""
    img, m, _ = C.levels_of(oracle, "noise", mname)
    r = _copy(ctx.orb_host(img, m, 2001))
    f = C.hold_request(r, oracle, "noise", mname, 2001, "noise, mask %s, 2001 features (three launches)" % mname)
    assert f["excess"] > 0, f["excess"]


def test_orb_slot_meets_the_definitions(ctx, oracle):
    img, _, _ = C.levels_of(oracle, "canvas", "none")
    assert ctx.upload_mono(3, img) == (160, 120)
    r = _copy(ctx.orb_slot(3, 300, 0))
    f = C.hold_request(r, oracle, "canvas", "none", 300, "slot path: canvas, 300 features")
    assert f["excess"] > 0 and f["n"] >= 100
    again = _copy(ctx.download_keypoints(3))
    assert all(np.array_equal(again[k], r[k]) for k in r), "the slot's keypoint arrays are not what orb_slot returned"


@pytest.mark.parametrize("iname", C.IMAGES)
def test_a_quarter_turn_and_a_mirror_image(ctx, iname):
    img = C.image(iname)

    def run(im):
        return _copy(ctx.orb_host(im, None, 4000))
    q, mi = C.quarter_turn(run, img), C.mirror(run, img)
    print("%s: quarter turn of %d keypoints: angles within %.2g deg, %d bits differ (all at rounding ties); mirror: angles within %.2g deg"
          % (iname, q["n"], q["angle"], q["bits_differ"], mi["angle"]))
    assert q["n"] >= 100
