"""MODE_SGBM_3WAY (mode 2) on the CPU: the cases of tests/sgbm_3way_def.py hold their coverage conditions on the definition alone,
and the evidence that a comparison with that definition can fail:

    coverage          every case of CASES3 holds the conditions of its scene (hold_coverage3)
    direction sets    seven wrong direction sets -- a path missing, S for N, a diagonal for N, N counted twice -- each change the
                      final image of we2-96x21
    twins             every layered case differs from the same pair in the mode (0 or 1) its twin in sgbm_def_cases runs: a
                      device that silently ran five or eight paths fails tests/test_gpu_sgbm_3way.py
    quality           valid share, rejects and the distance to MODE_HH on one SYNTHETIC corridor pair (C1, pair 3, 640 x 480,
                      D = 64, after median3, no speckle filter), printed as the table of the README; asserted: mode 2 keeps
                      >= 0.95 of mode 0's valid share
    binding           the cv2_compat constants, StereoSGBM_create(mode=2) and features.StereoSGBM down to set_sgbm(..., 2) on a
                      stand-in context, and a parameter file with and without "mode" through save_files / from_files / from_pfiles

tests/test_gpu_sgbm_3way.py holds csrc/sgbm.hip + sgbm_vert.inc to the same definition on the same cases."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402
import sgbm_3way_def as T          # noqa: E402

WRONG_SETS = (("W", "E"), ("W", "N"), ("N", "E"), ("W", "S", "E"), ("W", "NW", "E"), ("W", "NE", "E"), ("W", "N", "E", "N"))


def test_the_cases_are_the_device_cases_of_the_five_and_eight_path_suite():
    keys = {(c.scene, c.w, c.h, c.seed if c.name != "block7-minD0" else 0) + tuple(sorted(c.p.items())) for c in T.CASES3}
    want = {(c.scene, c.w, c.h, c.seed) + tuple(sorted(c.p.items())) for c in C.CASES if c.gpu and c.waves is None}
    assert keys == want and len(T.CASES3) == len(want) == 37
    assert all(c.mode == 2 and c.gpu and c.waves is None for c in T.CASES3)
    scheds = {s: sum(c.sched == s for c in T.CASES3) for s in (T.VERT, T.VERT_RAGGED, T.UNFUSED)}
    print("schedules: %s" % scheds)
    assert all(n >= 1 for n in scheds.values())
    # W + E by each of its three kernels, every register count, padded and exact ranges
    W1 = [DEF.effective(c.p, c.w).W1 for c in T.CASES3 if c.sched != T.UNFUSED]
    assert any(w % 16 == 0 and w >= 32 for w in W1) and any(w % 8 == 0 and w >= 16 and not (w % 16 == 0 and w >= 32) for w in W1)
    assert {(c.p["numDisparities"] + 31) // 32 for c in T.CASES3} == set(range(1, 9))
    assert {16, 48, 112} <= {c.p["numDisparities"] for c in T.CASES3}


@pytest.mark.parametrize("name", T.NAMES3)
def test_every_case_holds_its_conditions(name):
    c = T.BY_NAME3[name]
    T.hold_coverage3(c)
    d = T.definition3(c)[0]
    print(T.figures3(c))
    assert d["S"].max() <= DEF.MAX_S and d["S"].min() >= 0


def test_wrong_direction_sets_are_told_from_the_definition():
    c = T.BY_NAME3["we2-96x21"]
    L, R = C.images(c)
    want = T.definition3(c)[0]["final"]
    for dirs in WRONG_SETS:
        n = int((T.compute3(L, R, c.p, dirs=dirs)["final"] != want).sum())
        print("(%s): %d pixels differ from (W, N, E)" % (", ".join(dirs), n))
        assert n >= 1, dirs
    # and the order of the sum means nothing
    assert np.array_equal(T.compute3(L, R, c.p, dirs=("E", "W", "N"))["final"], want)


@pytest.mark.parametrize("name", [c.name for c in T.CASES3 if c.scene == "layered"])
def test_layered_cases_differ_from_their_twin_of_five_or_eight_paths(name):
    c = T.BY_NAME3[name]
    twin_mode = next(o.mode for o in C.CASES if T._name(o.name) == name and o.gpu and o.waves is None)
    twin = C.definition(c._replace(mode=twin_mode))[0]["final"]
    n = int((twin != T.definition3(c)[0]["final"]).sum())
    print("%s: %d pixels differ from mode %d" % (name, n, twin_mode))
    assert n >= 1


def test_quality_on_one_synthetic_corridor_pair():
    """The table of the README: this project's own path-wise definition on ONE SYNTHETIC pair, not real footage."""
    from openvo_amd.synth import Corridor
    co = Corridor("C1")
    L, R = co.pair(3)
    p = dict(co.sgbm_params(), speckleWindowSize=0)
    assert L.shape == (480, 640) and p["numDisparities"] == 64
    e = DEF.effective(p, co.w)
    Cv = DEF.cost_volume(L, R, p)
    S, sums = 0, {}
    for n in ("W", "N", "E", "NW", "NE", "SW", "S", "SE"):          # one volume at a time: 3WAY, SGBM and HH are prefixes of this order
        S = S + DEF.path(Cv, *DEF.DIRS[n], e.P1, e.P2)
        if n in ("E", "NE", "SE"):
            sums[{"E": "3WAY (W, E, N)", "NE": "SGBM (5)", "SE": "HH (8)"}[n]] = np.minimum(S, DEF.MAX_S)
    del S, Cv
    rows = {}
    for what, Sm in sums.items():
        info = {}
        med = DEF.median3(DEF.wta(Sm, e, co.w, info=info))[:, e.x0:e.x1]
        rows[what] = (med, med >= e.minD * 16, info)
    hh, hh_ok = rows["HH (8)"][0], rows["HH (8)"][1]
    print("paths | valid share of the band | uniqueness rejects | left-right rejects | valid in both (this, HH) | of those, > 1 px off MODE_HH | mean abs. difference to MODE_HH")
    for what in ("HH (8)", "SGBM (5)", "3WAY (W, E, N)"):
        med, ok, info = rows[what]
        both = ok & hh_ok
        diff = np.abs(med[both].astype(np.int64) - hh[both]) / 16.0
        print("%s | %.3f | %d | %d | %.3f | %.2f %% | %.3f px" % (what, ok.mean(), info["uniqueness"], info["left_right"], both.mean(),
                                                                 100 * (diff > 1).mean(), diff.mean()))
    share3, share5 = rows["3WAY (W, E, N)"][1].mean(), rows["SGBM (5)"][1].mean()
    assert share3 >= 0.95 * share5, (share3, share5)


# ---- binding ----------------------------------------------------------------------------------------------------------------
class _StandIn:
    """what cv2_compat / features ask of a context, recording what reaches set_sgbm"""

    def __init__(self):
        self.calls = []

    def set_sgbm(self, p, mode=0):
        self.calls.append((dict(p), int(p.get("mode", mode))))             # (the rule of _native.Context.set_sgbm)

    def sgbm_compute_host(self, left, right):
        return np.zeros(left.shape, np.int16)


def test_cv2_compat_carries_the_mode_constants_and_passes_the_mode_down(monkeypatch):
    from openvo_amd import cv2_compat as shim, features
    assert (shim.STEREO_SGBM_MODE_SGBM, shim.STEREO_SGBM_MODE_HH, shim.STEREO_SGBM_MODE_SGBM_3WAY) == (0, 1, 2)
    assert (shim.StereoSGBM_MODE_SGBM, shim.StereoSGBM_MODE_HH, shim.StereoSGBM_MODE_SGBM_3WAY) == (0, 1, 2)
    ctx = _StandIn()
    monkeypatch.setattr(shim, "_context", lambda *a, **k: ctx)
    img = np.zeros((16, 48), np.uint8)
    shim.StereoSGBM_create(0, 16, 5, mode=shim.STEREO_SGBM_MODE_SGBM_3WAY).compute(img, img)
    shim.StereoSGBM_create(0, 16, 5).compute(img, img)                      # nothing changes for a caller who passes no mode
    assert [m for _, m in ctx.calls] == [2, 0]
    p = C.params(16)
    features.StereoSGBM(ctx, dict(p, mode=2))
    features.StereoSGBM(ctx, p)
    assert [m for _, m in ctx.calls[2:]] == [2, 0]


def test_native_mode_constants_and_schedules():
    from openvo_amd import _native
    assert (_native.SCHED_DIAG, _native.SCHED_DIAG_RAGGED, _native.SCHED_UNFUSED, _native.SCHED_VERT, _native.SCHED_VERT_RAGGED) == (1, 2, 3, 4, 5)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vo355.h")).read()
    assert "VO_SCHED_VERT = 4" in header and "VO_SCHED_VERT_RAGGED = 5" in header


@pytest.mark.parametrize("ext", ["json", "npz"])
def test_a_parameter_file_round_trips_its_mode(tmp_path, ext):
    from openvo_amd import StereoCamera

    class Probe(StereoCamera):
        def __init__(self, *a, **k):
            self.args = a

    K, dist, rect = np.eye(3), np.zeros(5), {"R": np.eye(3), "T": np.array([-0.5, 0.0, 0.0])}
    base = C.params(64)
    for sgbm, mode in ((dict(base, mode=2), 2), (dict(base, mode=1), 1), (base, None)):
        files = [str(tmp_path / ("%s_%s.%s" % (n, mode, ext))) for n in ("l", "r", "rect", "sgbm")]
        StereoCamera.save_files(*files, K, dist, K, dist, rect, sgbm)
        got = Probe.from_files(*files, (64, 48)).args[5]
        assert got == sgbm and ("mode" in got) == (mode is not None)
        ctx = _StandIn()
        ctx.set_sgbm(got)
        assert ctx.calls[0][1] == (mode or 0)                               # a file without a mode reads as mode 0
        pf = []
        for n, d in zip(("l", "r", "rect", "sgbm"), ({"K": K, "dist": dist}, {"K": K, "dist": dist}, rect, sgbm)):
            pf.append(str(tmp_path / ("%s_%s_%s.p" % (n, mode, ext))))
            with open(pf[-1], "wb") as fh:
                pickle.dump(d, fh)
        assert Probe.from_pfiles(*pf, (64, 48)).args[5] == sgbm
