"""The Lucas-Kanade PnP pair step without a GPU: the three entries are exported and bound with the argument counts of
include/vo355.h, StereoOdometer(klt_fused=True) is refused outside match="klt" / pose_method="pnp", and an odometer built without
the keyword is the object it was."""
import ctypes
import os
import re
import types

import pytest

from openvo_amd import StereoOdometer, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"vo_klt_pnp_pair": 25, "vo_klt_pnp_pair_begin": 17, "vo_klt_pnp_pair_end": 12}


def _header_arg_counts():
    txt = open(os.path.join(ROOT, "include", "vo355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: len(args.split(",")) for name, args in re.findall(r"\bint\s+(vo_klt_pnp_pair\w*)\s*\(([^)]*)\)\s*;", txt)}


def test_the_entries_are_declared_exported_and_bound_with_their_argument_counts():
    assert _header_arg_counts() == ENTRIES
    _native.build_native()
    L = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, n in ENTRIES.items():
        assert name in _native.SYMBOLS and hasattr(raw, name)
        assert len(getattr(L, name).argtypes) == n, name
    for name in ("klt_pnp_pair", "klt_pnp_pair_begin", "klt_pnp_pair_end"):
        assert callable(getattr(_native.Context, name))
    # the product library has no planting seam
    assert not hasattr(raw, "vo_test_plant_dense_pair")


def test_the_binding_refuses_what_the_library_would():
    """checked before the library is called: no context is needed"""
    c = _native.Context.__new__(_native.Context)
    c._h = None
    K4 = (100.0, 100.0, 50.0, 40.0)
    for kw in (dict(win=22), dict(levels=0), dict(fb=-1.0), dict(klt_iters=0), dict(lo_rounds=1), dict(lo_rounds=9, refine=3)):
        with pytest.raises(ValueError):
            c._klt_pnp_front(0, 1, K4, 256, 1.5, 4321, kw.pop("refine", 0), kw.pop("lo_rounds", 0), kw)
    front, _ = c._klt_pnp_front(0, 1, K4, 256, 1.5, 4321, 3, 2, dict(win=9, levels=2, klt_iters=7, fb=0.0))
    assert front[1:9] == [0, 1, 9, 2, 7, 0.01, 1e-4, 0.0] and front[10:] == [256, 1.5, 4321, 3, 2]


def _odometer(**kw):
    return StereoOdometer(types.SimpleNamespace(), **kw)


def test_constructor_refusals():
    for kw in (dict(match="orb"), dict(match="klt", pose_method="umeyama"), dict(match="orb", pose_method="pnp"), dict()):
        with pytest.raises(ValueError, match="klt_fused"):
            _odometer(klt_fused=True, **kw)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="klt_fused"):
            _odometer(match="klt", pose_method="pnp", klt_fused=bad)


def test_a_default_odometer_is_the_object_it_was():
    for kw in (dict(), dict(match="klt", pose_method="pnp"), dict(match="klt")):
        o = _odometer(**kw)
        assert "klt_fused" not in o.__dict__ and not hasattr(o, "klt_ahead") and o.klt_fused is False
    o = _odometer(match="klt", pose_method="pnp", klt_fused=True)
    assert o.__dict__["klt_fused"] is True and o.klt_ahead == 0 and o.klt_counts is None


def test_the_key_of_a_step_begun_ahead_carries_the_tracker():
    import numpy as np
    Q = np.eye(4)
    Q[0, 3], Q[1, 3], Q[2, 3] = -320.0, -240.0, 500.0
    keys = []
    for kw in (dict(), dict(klt_window=9), dict(klt_levels=2), dict(klt_fb=0.0)):
        o = StereoOdometer(types.SimpleNamespace(Q=Q), match="klt", pose_method="pnp", klt_fused=True, **kw)
        keys.append(o._pose_params())
        kwargs = StereoOdometer._klt_kwargs(keys[-1])
        assert (kwargs["win"], kwargs["levels"], kwargs["fb"]) == (o.klt_window, o.klt_levels, o.klt_fb)
        assert kwargs["K4"] == (500.0, 500.0, 320.0, 240.0)
    assert len(set(keys)) == 4 and all(k[0] == "klt" for k in keys)
