"""Host logic of the landmark map's public arguments (no GPU): the constructor's validation, track="pair" standing exactly where
the odometer stood before the map existed, the reserved view slot, and header / binding agreement on the vo_map_* entries."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_ENTRIES = ("vo_map_create", "vo_map_destroy", "vo_map_reset", "vo_map_view", "vo_map_update", "vo_map_download")
MAP_METHODS = ("map_create", "map_destroy", "map_reset", "map_view", "map_update", "map_download")
NEW_ATTRS = {"track", "map_max_age", "map_capacity", "map_max_obs", "map_z_min", "track_source", "map_counts", "_map", "_view_slot", "_map_serial"}


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])


def test_track_and_its_requirements():
    from openvo_amd import StereoOdometer
    assert StereoOdometer(_Cam()).track == "pair"
    odo = StereoOdometer(_Cam(), track="map", depth="sparse", pose_method="pnp")
    assert (odo.track, odo.map_max_age, odo.map_capacity, odo.map_max_obs, odo.map_z_min) == ("map", 5, None, 8, 0.1)
    assert odo.track_source is None and odo.map_counts == {}
    for bad in ("Map", "", None, 1, True, b"map"):
        with pytest.raises(ValueError, match="track"):
            StereoOdometer(_Cam(), track=bad, depth="sparse", pose_method="pnp")
    for kw in (dict(), dict(depth="dense", pose_method="pnp"), dict(depth="sparse"), dict(depth="sparse", pose_method="umeyama"),
               dict(depth="dense", pose_method="umeyama")):
        with pytest.raises(ValueError, match="track='map' needs"):
            StereoOdometer(_Cam(), track="map", **kw)


@pytest.mark.parametrize("track", ["pair", "map"])
def test_map_arguments_are_validated(track):
    from openvo_amd import StereoOdometer
    base = dict(track=track, depth="sparse", pose_method="pnp")
    for bad in (-1, 1.0, "5", None, True):
        with pytest.raises(ValueError, match="map_max_age"):
            StereoOdometer(_Cam(), map_max_age=bad, **base)
    for bad in (0, -3, 65536, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="map_max_obs"):
            StereoOdometer(_Cam(), map_max_obs=bad, **base)
    for bad in (15, 0, -1, 2000.0, "2000", True):
        with pytest.raises(ValueError, match="map_capacity"):
            StereoOdometer(_Cam(), map_capacity=bad, **base)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, "0.1", None, True):
        with pytest.raises(ValueError, match="map_z_min"):
            StereoOdometer(_Cam(), map_z_min=bad, **base)
    odo = StereoOdometer(_Cam(), map_max_age=0, map_max_obs=65535, map_capacity=16, map_z_min=0, **base)
    assert (odo.map_max_age, odo.map_max_obs, odo.map_capacity, odo.map_z_min) == (0, 65535, 16, 0.0)


def test_pair_mode_stands_where_it_stood():
    """track="pair": every attribute the odometer had before the map existed, with the value it had, and _pose_params() of both pose
    methods -- the new names aside, nothing else appeared."""
    from openvo_amd import StereoOdometer
    from openvo_amd.stereo_odometer import LoopCheck
    cam = _Cam()
    odo = StereoOdometer(cam)
    had = dict(depth="dense", sparse_row_tol=2.0, sparse_max_hamming=75, sparse_mutual=False, sparse_ratio=None, loop_check=None,
               cross_check=False, match_window=None, _pair_span=None, pnp_refine=0, pose_method="umeyama", pnp_iters=256, pnp_threshold=1.5,
               pnp_seed=4321, stereo=cam, current_img=None, current_disparity=None, current_3d=None, prev_img=None, prev_disparity=None,
               prev_3d=None, _ctx=None, orb=None, matcher=None, prev_kps=None, current_kps=None, current_desc=None, match_threshold=0.8,
               rigidity_threshold=0, outlier_threshold=0, preprocessed_frames=False, min_matches=10, skipped_frames=0, skip_cause="",
               _specs={}, _next_hint=(), _ahead_counts={})
    got = vars(odo)
    assert set(got) - NEW_ATTRS == set(had) | {"c_T_w", "c_T_w_prev", "pose_ahead"}, sorted(set(got) ^ (set(had) | NEW_ATTRS))
    for k, v in had.items():
        assert got[k] is v or got[k] == v, k
    assert np.array_equal(odo.c_T_w, np.eye(4)) and np.array_equal(odo.c_T_w_prev, np.eye(4))
    assert odo._pose_params() == (0.8, 10, 0.0, 0.0, False)
    pnp = StereoOdometer(cam, pose_method="pnp", depth="sparse", pnp_refine=3, cross_check=True, match_window=(30, 20), loop_check=40)
    want = ("pnp", 0.8, (400.0, 400.0, 320.0, 240.0), 256, 1.5, 4321, 3, True, (30.0, 20.0), LoopCheck(40))
    assert pnp._pose_params() == want
    assert StereoOdometer(cam, pose_method="pnp", depth="sparse", pnp_refine=3, cross_check=True, match_window=(30, 20), loop_check=40,
                          track="map")._pose_params() == want          # the map step IS that PnP step
    with pytest.raises(ValueError, match="track='map'"):
        odo.landmarks()


def test_the_view_slot_is_set_aside():
    """reserve_view_slot: never handed out, not counted as a look-ahead pair, given back by release_view_slot"""
    from openvo_amd import _native
    from openvo_amd.stereo_camera import StereoCamera, _RESERVED
    cam = StereoCamera.__new__(StereoCamera)
    n = _native.VO_NUM_SLOTS
    cam._slot_owner, cam._slot_gen, cam._next_slot, cam._lookahead = [None] * n, [0] * n, 0, []
    v = cam.reserve_view_slot()
    assert v == 0 and cam._slot_gen[v] == 1
    handed = [cam._free_slot() for _ in range(2 * n)]
    assert v not in handed and set(handed) == set(range(n)) - {v}
    assert sum(1 for o in cam._slot_owner if o is _RESERVED) == 0
    for s in range(n):
        if s != v:
            cam._slot_owner[s] = _RESERVED
    assert cam._free_slot() is None
    with pytest.raises(RuntimeError):
        cam._acquire_slot()                    # every other slot holds a submitted pair: the view slot is not evicted either
    cam.release_view_slot(v)
    cam.release_view_slot(v)
    assert cam._free_slot() == v


def test_map_symbols_and_header_lines():
    from openvo_amd import _native
    header = open(os.path.join(ROOT, "include", "vo355.h")).read()
    assert "NOT part of the reference" in header[header.index("Landmark map"):header.index("int vo_map_create")]
    assert re.search(r"^#define VO_NUM_MAPS 4$", header, re.M) and _native.VO_NUM_MAPS == 4
    for name in MAP_ENTRIES:
        assert name in _native.SYMBOLS
        assert re.search(r"^int %s\(vo_ctx\* ctx," % name, header, re.M), name
    declared = set(re.findall(r"^int (vo_map_[a-z_]+)\(", header, re.M))
    assert declared == set(MAP_ENTRIES) == {s for s in _native.SYMBOLS if s.startswith("vo_map_")}
    for method in MAP_METHODS:
        assert callable(getattr(_native.Context, method))
    if os.path.exists(_native.LIB_PATH):
        lib = _native.lib()
        for name in MAP_ENTRIES:
            assert hasattr(lib, name), name
            assert getattr(lib, name).argtypes is not None, name
        assert not hasattr(lib, "vo_test_plant_map")           # the planting seam lives in the test-only library alone
