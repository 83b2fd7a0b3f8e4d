"""The SGBM cost option (vo_set_sgbm_cost) on the host side, no device: the three ABI names, the parameter keys through
StereoCamera's files, cv2_compat and features.StereoSGBM, and the census settings of the synthetic corridor."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_def_cases as C         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vo_set_sgbm_cost", "vo_get_sgbm_cost", "vo_sgbm_cost_volume")


def test_the_abi_names_are_in_the_table_and_in_the_header():
    from openvo_amd import _native
    header = open(os.path.join(ROOT, "include", "vo355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert n in _native.SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
    assert re.search(r"#define\s+VO_SGBM_COST_BT\s+0\b", code) and re.search(r"#define\s+VO_SGBM_COST_CENSUS\s+1\b", code)
    assert (_native.COST_BT, _native.COST_CENSUS) == (0, 1)
    for m in ("set_sgbm_cost", "sgbm_cost", "sgbm_cost_volume"):
        assert callable(getattr(_native.Context, m))


class _StandIn:
    def __init__(self):
        self.calls = []

    def set_sgbm(self, p, mode=0):
        self.calls.append(dict(p))

    def sgbm_compute_host(self, left, right):
        return np.zeros(left.shape, np.int16)


def test_cv2_compat_and_features_carry_the_cost(monkeypatch):
    from openvo_amd import cv2_compat as shim, features
    assert (shim.STEREO_SGBM_COST_BT, shim.STEREO_SGBM_COST_CENSUS) == (0, 1)
    ctx = _StandIn()
    monkeypatch.setattr(shim, "_context", lambda *a, **k: ctx)
    img = np.zeros((16, 48), np.uint8)
    s = shim.StereoSGBM_create(0, 16, 5, cost=shim.STEREO_SGBM_COST_CENSUS)
    assert (s.params["cost"], s.params["censusWidth"], s.params["censusHeight"]) == (1, 9, 7)
    s.compute(img, img)
    shim.StereoSGBM_create(0, 16, 5, cost=1, censusWidth=5, censusHeight=3).compute(img, img)
    shim.StereoSGBM_create(0, 16, 5).compute(img, img)                      # nothing changes for a caller who passes no cost
    assert [(p["cost"], p["censusWidth"], p["censusHeight"]) for p in ctx.calls] == [(1, 9, 7), (1, 5, 3), (0, 9, 7)]
    p = C.params(16)
    a = features.StereoSGBM(ctx, dict(p, cost=1, censusWidth=7, censusHeight=5))
    b = features.StereoSGBM(ctx, p)
    assert (a.cost, a.census_window, b.cost, b.census_window) == (1, (7, 5), 0, (9, 7))
    assert ctx.calls[3]["cost"] == 1 and "cost" not in ctx.calls[4]          # a dict without the key reaches set_sgbm without it: BT


@pytest.mark.parametrize("ext", ["json", "npz"])
def test_a_parameter_file_round_trips_the_cost_keys(tmp_path, ext):
    from openvo_amd import StereoCamera
    assert set(StereoCamera.SGBM_OPTIONAL_KEYS) >= {"mode", "cost", "censusWidth", "censusHeight"}

    class Probe(StereoCamera):
        def __init__(self, *a, **k):
            self.args = a

    K, dist, rect = np.eye(3), np.zeros(5), {"R": np.eye(3), "T": np.array([-0.5, 0.0, 0.0])}
    base = C.params(64)
    for i, sgbm in enumerate((dict(base, cost=1, censusWidth=9, censusHeight=3), dict(base, cost=1, mode=2), dict(base, cost=0), base)):
        files = [str(tmp_path / ("%s_%d.%s" % (n, i, ext))) for n in ("l", "r", "rect", "sgbm")]
        StereoCamera.save_files(*files, K, dist, K, dist, rect, sgbm)
        got = Probe.from_files(*files, (64, 48)).args[5]
        assert got == sgbm and all(isinstance(v, int) for v in got.values())
        pf = []
        for n, d in zip(("l", "r", "rect", "sgbm"), ({"K": K, "dist": dist}, {"K": K, "dist": dist}, rect, sgbm)):
            pf.append(str(tmp_path / ("%s_%d_%s.p" % (n, i, ext))))
            with open(pf[-1], "wb") as fh:
                pickle.dump(d, fh)
        assert Probe.from_pfiles(*pf, (64, 48)).args[5] == sgbm


def test_the_corridor_offers_the_census_settings():
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    bt, ce = c.sgbm_params(), c.sgbm_params(cost=1)
    assert "cost" not in bt and c.sgbm_params(cost=0) == dict(bt, cost=0)
    assert ce == dict(bt, cost=1, censusWidth=9, censusHeight=7, P1=50, P2=200)
    assert c.sgbm_params(2, cost=1)["mode"] == 2 and c.sgbm_params(2) == dict(bt, mode=2)
