"""Host side of the fused map step (no GPU): the constructor's option, the native calls StereoOdometer._map_track makes with and
without it (counted on a stand-in context, every call bound against the real binding's signature), what it does with the record,
and header / binding agreement on vo_track_map."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from openvo_amd import StereoOdometer, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(track="map", depth="sparse", pose_method="pnp")


class _Cam:
    _ctx = None
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])

    def slot_key(self, s):
        return (s, 0)


# ---- the option --------------------------------------------------------------------------------------------------------------------
def test_map_fused_and_its_requirement():
    assert StereoOdometer(_Cam()).map_fused is False and StereoOdometer(_Cam(), **BASE).map_fused is False
    assert StereoOdometer(_Cam(), map_fused=False).map_fused is False
    assert "map_fused" not in vars(StereoOdometer(_Cam(), **BASE))          # off: the object is what it was
    assert StereoOdometer(_Cam(), map_fused=True, **BASE).map_fused is True
    assert StereoOdometer(_Cam(), map_fused=np.True_, **BASE).map_fused is True
    for kw in (dict(), dict(track="pair"), dict(track="pair", depth="sparse", pose_method="pnp")):
        with pytest.raises(ValueError, match="map_fused=True needs track='map'"):
            StereoOdometer(_Cam(), map_fused=True, **kw)
    for bad in (1, 0, "True", None, 1.0):
        with pytest.raises(ValueError, match="map_fused"):
            StereoOdometer(_Cam(), map_fused=bad, **BASE)
    assert inspect.signature(StereoOdometer.__init__).parameters["map_fused"].default is False


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def _bound(fn, *a, **kw):
    b = inspect.signature(getattr(_native.Context, fn)).bind(None, *a, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k != "self"}


def _rt(angle, dist):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, dist], [0, 1, 0, 0], [-s, 0, c, 0]], np.float64)


WIN = _rt(0.01, 0.20)
CW = np.array([[0.5, 0, 0, 1.0], [0, 0.25, 0, 2.0], [0, 0, 2.0, 3.0]])        # (no rotation: only ever copied)


class _Ctx:
    """stands in for _native.Context: counts the map and PnP calls and hands out scripted results"""
    kp_cap = 3024

    def __init__(self, size=1200, vis=900, decision=0, flags=0):
        self.calls, self.size, self.vis, self.decision, self.flags = [], size, vis, decision, flags

    def map_view(self, *a, **kw):
        self.calls.append(("map_view", _bound("map_view", *a, **kw)))
        return np.array([self.size, self.vis], np.int32)

    def _pnp(self):
        return dict(matches=50, n=40, best_iter=7, best_count=30, flags=0, Rt=WIN, Rt_refined=WIN, refine_status=1, refine_steps=0,
                    q=np.arange(40, dtype=np.int32), t=np.arange(40, dtype=np.int32), mask=np.ones(40, np.uint8))

    def pnp_pair(self, *a, **kw):
        self.calls.append(("pnp_pair", _bound("pnp_pair", *a, **kw)))
        return self._pnp()

    def pnp_pair_window(self, *a, **kw):
        self.calls.append(("pnp_pair_window", _bound("pnp_pair_window", *a, **kw)))
        return self._pnp()

    def map_update(self, *a, **kw):
        self.calls.append(("map_update", _bound("map_update", *a, **kw)))
        self.size += 7
        return np.array([30, 0, 3, 10, 0, self.size], np.int32)

    def map_track(self, *a, **kw):
        self.calls.append(("map_track", _bound("map_track", *a, **kw)))
        ok = self.decision == 0
        if ok:
            self.size += 7
        return dict(self._pnp(), decision=self.decision, flags=self.flags, view=np.array([self.size - 7 * ok, self.vis], np.int32), update_flags=0,
                    update=np.array([30, 0, 3, 10, 0, self.size], np.int32) if ok else np.full(6, -1, np.int32),
                    c_T_w=CW if ok else np.zeros((3, 4)), w_T_c=np.zeros((3, 4)))

    @staticmethod
    def rodrigues(R):
        return _native.Context.rodrigues(R)


class _Frame:
    slot = 5


class _Kps:
    frame = _Frame()

    def __init__(self, n=600):
        self.n = n

    def __len__(self):
        return self.n


def _odo(ctx, size=None, **kw):
    od = StereoOdometer(_Cam(), **dict(BASE, **kw))
    od._ctx, od._map, od._view_slot, od.skip_cause = ctx, 2, 9, "init"
    od._map_ready = lambda *a: None              # (the stand-in frames are not device frames)
    od._map_size = ctx.size if size is None else size
    od._map_serial = 4
    od.c_T_w = np.vstack([_rt(0.3, 2.0), [0, 0, 0, 1]])
    return od


def test_without_the_option_the_step_makes_the_calls_it_made():
    ctx = _Ctx()
    od = _odo(ctx)
    before = od.c_T_w.copy()
    assert od._map_track(_Kps(), None, None) is True
    assert [c[0] for c in ctx.calls] == ["map_view", "pnp_pair", "map_update"]
    view, pnp, upd = (c[1] for c in ctx.calls)
    assert (view["handle"], view["ref_slot"], view["view_slot"], view["z_min"]) == (2, 5, 9, 0.1) and np.array_equal(view["Rt_cw"], before)
    assert (pnp["slot_a"], pnp["slot_b"], pnp["want_matches"]) == (9, 5, True)
    assert (upd["handle"], upd["slot_new"], upd["serial"], upd["max_age"], upd["max_obs"]) == (2, 5, 4, 5, 8) and len(upd["q"]) == 40
    assert np.array_equal(upd["Rt_wc"], np.linalg.inv(np.vstack([WIN, [0, 0, 0, 1]]) @ before))
    assert np.array_equal(od.c_T_w, np.vstack([WIN, [0, 0, 0, 1]]) @ before) and od.track_source == "map" and od._map_serial == 5
    # with a window the PnP step is the _window form, as ever; a view too small ends the step behind map_view
    ctx = _Ctx()
    assert _odo(ctx, match_window=(30, 20))._map_track(_Kps(), None, None) is True
    assert [c[0] for c in ctx.calls] == ["map_view", "pnp_pair_window", "map_update"]
    ctx = _Ctx(vis=9)
    assert _odo(ctx)._map_track(_Kps(), None, None) is False and [c[0] for c in ctx.calls] == ["map_view"]


@pytest.mark.parametrize("skipped", [0, 2])
def test_with_the_option_the_step_is_one_call(skipped):
    ctx = _Ctx()
    od = _odo(ctx, map_fused=True, cross_check=True, match_window=(30, 20), loop_check=40, pnp_refine=3, min_matches=12)
    od.skipped_frames = skipped
    before = od.c_T_w.copy()
    assert od._map_track(_Kps(), None, None) is True
    assert [c[0] for c in ctx.calls] == ["map_track"]
    a = ctx.calls[0][1]
    span = skipped + 1
    assert (a["handle"], a["slot_new"], a["view_slot"], a["z_min"], a["serial"], a["max_age"], a["max_obs"]) == (2, 5, 9, 0.1, 4, 5, 8)
    assert np.array_equal(a["Rt_cw_pred"], before) and tuple(a["K4"]) == (400.0, 400.0, 320.0, 240.0)
    assert (a["ratio"], a["iters"], a["thr"], a["seed"], a["refine"], a["min_matches"]) == (0.8, 256, 1.5, 4321, 3, 12)
    assert a["max_dist"] == StereoOdometer.MAX_DISTANCE_CHANGE * span and a["max_rot"] == StereoOdometer.MAX_ROTATION_CHANGE * span
    assert a["cross_check"] is True and a["loop"] == 40
    assert a["window"] == tuple(float(np.float32(r * span)) for r in (30, 20))          # the window scales with the span, as ever
    assert np.array_equal(od.c_T_w, np.vstack([CW, [0, 0, 0, 1]])) and np.array_equal(od.c_T_w_prev, before)
    assert od.track_source == "map" and od._map_serial == 5 and od.skip_cause == "init"
    assert tuple(od.map_counts["view"]) == (1200, 900) and tuple(od.map_counts["update"]) == (30, 0, 3, 10, 0, 1207) and od._map_size == 1207
    assert od._map_track(_Kps(), None, None) is True and [c[0] for c in ctx.calls] == ["map_track"] * 2 and ctx.calls[1][1]["serial"] == 5


@pytest.mark.parametrize("decision,cause", [(1, "init"), (2, "matches"), (3, "matches"), (4, "outlier"), (5, "nan"), (6, "bigdist"), (7, "bigrot")])
def test_decisions_become_skip_causes_and_nothing_else_changes(decision, cause):
    ctx = _Ctx(decision=decision)
    od = _odo(ctx, map_fused=True)
    before = (od.c_T_w.copy(), od.c_T_w_prev.copy())
    assert od._map_track(_Kps(), None, None) is False
    assert [c[0] for c in ctx.calls] == ["map_track"] and od.skip_cause == cause
    assert np.array_equal(od.c_T_w, before[0]) and np.array_equal(od.c_T_w_prev, before[1])
    assert od.track_source is None and od._map_serial == 4 and "update" not in od.map_counts and tuple(od.map_counts["view"]) == (1200, 900)
    assert set(_native.MAP_DECISIONS) == set(range(8))


def test_lookup_flag_raises_behind_the_match_count():
    with pytest.raises(ZeroDivisionError):
        _odo(_Ctx(decision=0, flags=1), map_fused=True)._map_track(_Kps(), None, None)
    od = _odo(_Ctx(decision=2, flags=1), map_fused=True)
    assert od._map_track(_Kps(), None, None) is False and od.skip_cause == "matches"


def test_a_map_beyond_the_fused_bound_takes_the_unfused_chain():
    assert _native.MAP_TRACK_MAX == 3800
    ctx = _Ctx(size=3801, vis=900)
    assert _odo(ctx, map_fused=True)._map_track(_Kps(), None, None) is True
    assert [c[0] for c in ctx.calls] == ["map_view", "pnp_pair", "map_update"]
    ctx = _Ctx(size=3800, vis=900)
    assert _odo(ctx, map_fused=True)._map_track(_Kps(), None, None) is True and [c[0] for c in ctx.calls] == ["map_track"]
    # the size the odometer goes by is the one the folds report
    od = _odo(_Ctx(size=100), map_fused=True, size=0)
    od._map_fold(5)
    assert od._map_size == 107


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "vo355.h")).read()
    assert re.search(r"^#define VO_MAP_TRACK_MAX 3800$", header, re.M)
    decl = re.search(r"^int vo_track_map\((.*?)\);", header, re.M | re.S).group(1)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert len(params) == 24 and params[0] == "vo_ctx* ctx" and params[-1] == "int cap"
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
    struct = re.search(r"typedef struct vo_track_map_rec \{(.*?)\} vo_track_map_rec;", header, re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(int32_t|double) ([^;]+);", re.sub(r"/\*.*?\*/", "", struct, flags=re.S)):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            fields.append((m.group(1), typ, int(m.group(2) or 1)))
    got = [(n, "int32_t" if (t._type_ if hasattr(t, "_length_") else t) is ctypes.c_int32 else "double", getattr(t, "_length_", 1))
           for n, t in _native.MapTrackRec._fields_]
    assert got == fields and ctypes.sizeof(_native.MapTrackRec) == 20 * 4 + 48 * 8
    assert "vo_track_map" in _native.SYMBOLS and callable(_native.Context.map_track)
    # bound in the loop form of the other map entries: the misuse sweep, which draws from one random stream over the entries bound
    # attribute by attribute, calls what it called before
    src = open(_native.__file__).read()
    assert not re.search(r"L\.vo_track_map\.argtypes", src) and '("vo_track_map", [' in src
    if os.path.exists(_native.LIB_PATH):
        assert list(_native.lib().vo_track_map.argtypes) == want
