"""The fused map step on the CPU: known answers for its numpy restatement (tests/map_fused_ref.py) and, over the synthetic corridor,
the restated fused odometer against the unfused chain the tree already has (tests/map_ref.py, MapRefOdometer): the yardstick is
the existing restatement, not the code under test."""
import numpy as np
import pytest

import map_fused_ref as F
import map_ref as M

I34 = np.eye(4)[:3]
K4 = (400.0, 400.0, 320.0, 240.0)
CROP = (600, 440)
ORG = (20, 16)
MAXD, MAXR = 1.0, np.pi / 3


def _desc(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _planted(xyz, capacity=64, seed=0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    m = M.MapRef(capacity)
    m.plant(xyz, _desc(n, seed), _desc(n, seed + 1), np.arange(n) % 8, np.ones(n, np.int32), np.zeros(n, np.int32))
    return m


def _rt(angle, dist, axis=1):
    c, s = np.cos(angle), np.sin(angle)
    R = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.hstack([np.array(R, np.float64), [[dist], [0], [0]]])


# ---- decisions ---------------------------------------------------------------------------------------------------------------------
GOOD = dict(vis=100, matches=50, flags=0, n=40, best_count=30, T=_rt(0.01, 0.2), min_matches=10, max_dist=MAXD, max_rot=MAXR)


@pytest.mark.parametrize("change,code", [
    ({}, 0),
    (dict(vis=9), 1), (dict(vis=3801), 1), (dict(vis=1, min_matches=0), 1), (dict(vis=9, matches=0), 1),
    (dict(matches=9), 2), (dict(matches=9, flags=2), 2),
    (dict(flags=2), 8), (dict(flags=3, n=0), 8),
    (dict(n=9), 3), (dict(n=3, min_matches=2, matches=3, best_count=3), 3), (dict(n=9, best_count=0), 3),
    (dict(best_count=9), 4), (dict(best_count=9, T=np.full((3, 4), np.nan)), 4),
    (dict(T=np.full((3, 4), np.nan)), 5), (dict(T=np.where(np.arange(12).reshape(3, 4) == 6, np.nan, _rt(0.01, 0.2))), 5),
    (dict(T=_rt(0.01, 1.5)), 6), (dict(T=_rt(0.01, 2.5), max_dist=3.0), 0), (dict(T=_rt(0.01, 2.5), max_dist=2.0), 6),
    (dict(T=_rt(1.2, 0.2)), 7), (dict(T=_rt(1.2, 0.2, axis=0)), 7), (dict(T=_rt(-1.2, 0.2, axis=2)), 7), (dict(T=_rt(3.1, 0.2)), 7),
    (dict(T=_rt(1.2, 0.2), max_rot=2 * MAXR), 0),
    (dict(T=_rt(1.2, 1.5)), 7),                      # both gates: the last cause set wins
    (dict(flags=1), 0),                              # the lookup flag is the caller's business (it raises), not a decision
])
def test_decision_codes(change, code):
    assert F.decide(**dict(GOOD, **change)) == code


def test_gate_figures_are_norm_and_rotation_angle():
    for angle, axis in ((0.0, 1), (1e-9, 0), (0.3, 2), (-0.7, 1), (3.0, 0)):
        T = _rt(angle, 0.25, axis)
        T[:, 3] = [0.3, -0.4, 1.2]
        d, a = F.gate_figures(T)
        assert d == pytest.approx(1.3, abs=1e-15) and a == pytest.approx(abs(angle), abs=1e-12)
    assert sorted(set(F.CAUSES)) == list(range(8)) and F.CAUSES[1] is None and F.CAUSES[7] == "bigrot"


# ---- pose --------------------------------------------------------------------------------------------------------------------------
def test_compose_and_rigid_inverse_are_the_4x4_operations():
    rng = np.random.default_rng(5)
    for _ in range(20):
        T, P = _rt(rng.uniform(-1, 1), rng.uniform(-2, 2), int(rng.integers(3))), _rt(rng.uniform(-3, 3), rng.uniform(-50, 50), int(rng.integers(3)))
        P[:, 3] = rng.uniform(-80, 80, 3)
        cw = F.compose(T, P)
        want = (np.vstack([T, [0, 0, 0, 1]]) @ np.vstack([P, [0, 0, 0, 1]]))[:3]
        assert np.abs(cw - want).max() <= 4 * np.spacing(100.0)
        wc = F.rigid_inverse(cw)
        assert np.abs(wc - np.linalg.inv(np.vstack([cw, [0, 0, 0, 1]]))[:3]).max() <= 1e-12
        assert np.array_equal(wc[:, :3], cw[:, :3].T)
    # the bracketing: a case where left-to-right and any other order differ in the last bit
    T = np.array([[1e16, 1.0, -1e16, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]])
    P = np.array([[1.0, 0, 0, 0], [1.0, 1, 0, 0], [1.0, 0, 1, 0]])
    assert F.compose(T, P)[0, 0] == (1e16 + 1.0) - 1e16 == 0.0
    cw = np.array([[1.0, 0, 0, 1e16], [1.0, 1, 0, 1.0], [1.0, 0, 1, -1e16]])
    assert F.rigid_inverse(cw)[0, 3] == -(((1e16) + 1.0) + -1e16) == -0.0


# ---- padded view -------------------------------------------------------------------------------------------------------------------
def test_padded_view_is_the_view_then_clones_of_row_0():
    pts = [[0, 0, -2], [0.3, 0.1, 2], [np.nan, 0, 2], [0.1, 0, 2], [50, 0, 2], [0.2, 0.1, 3], [0, 0, 0.01]]      # the first and the last are invisible
    m, twin = _planted(pts), _planted(pts)
    want = twin.view(I34, K4, 0.1, ORG, CROP)
    v = F.padded_view(m, I34, K4, 0.1, ORG, CROP)
    assert v["vis"] == 3 and list(v["src"]) == [1, 3, 5] and list(m.view_src) == [1, 3, 5] and tuple(v["counts2"]) == (7, 3)
    for k in ("xy", "xyz", "desc", "rdesc", "octave"):
        assert len(v[k]) == 7 and v[k].dtype == want[k].dtype
        assert np.array_equal(v[k][:3], want[k]), k
    for k in ("xy", "desc", "rdesc", "octave"):
        assert all(np.array_equal(row, want[k][0]) for row in v[k][3:]), k
    assert np.isnan(v["xyz"][3:]).all()


def test_padded_view_of_nothing_visible_is_zero_filled():
    m = _planted([[0, 0, -2], [np.inf, 0, 1]])
    v = F.padded_view(m, I34, K4, 0.1, ORG, CROP)
    assert v["vis"] == 0 and len(v["xy"]) == 2 and not v["xy"].any() and not v["desc"].any() and not v["rdesc"].any() and not v["octave"].any()
    assert np.isnan(v["xyz"]).all()


# ---- device-fed update -------------------------------------------------------------------------------------------------------------
def _frame(xyz, seed=10):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    return dict(xyz=xyz, desc=_desc(n, seed), rdesc=_desc(n, seed + 1), octave=(np.arange(n) % 5).astype(np.int32))


def test_update_dev_applies_refuses_and_stands_back():
    pts = [[0, 0, 4], [0.01, 0, 4], [0, 0, -1]]
    f = _frame([[0, 0, 4.5], [1, 1, 5]])
    m, twin = _planted(pts), _planted(pts)
    assert F.padded_view(m, I34, K4, 0.1, ORG, CROP)["vis"] == 2 and len(twin.view(I34, K4, 0.1, ORG, CROP)["xy"]) == 2
    before = m.download()
    same = lambda: all(np.array_equal(before[k], m.download()[k], equal_nan=True) for k in M.FIELDS)     # noqa: E731
    c, fl = F.update_dev(m, f, I34, 1, 5, 8, [0], [0], [1], 2, accept=False)
    assert list(c) == [-1] * 6 and fl == 0 and same() and len(m.view_src) == 2
    for q, t, mask in (([2], [0], [1]), ([-1], [0], [1]), ([0], [2], [1]), ([0], [-1], [1]), ([0, 5], [0, 1], [1, 1])):
        c, fl = F.update_dev(m, f, I34, 1, 5, 8, q, t, mask, 2, accept=True)
        assert list(c) == [-1] * 6 and fl == 1 and same(), (q, t)
    # an entry that is no inlier is not an observation: whatever it names
    c, fl = F.update_dev(m, f, I34, 1, 5, 8, [0, 7, -3], [0, 9, 1], [1, 0, 0], 2, accept=True)
    want = twin.update(f, I34, 1, 5, 8, [0], [0], [1])
    assert fl == 0 and np.array_equal(c, want) and tuple(c) == (1, 0, 0, 1, 0, 4)
    assert all(np.array_equal(m.download()[k], twin.download()[k], equal_nan=True) for k in M.FIELDS)


def test_track_on_an_empty_map_and_on_a_map_too_large():
    r = F.track(M.MapRef(16), _frame([[0, 0, 4]]), I34, K4, 0.1, ORG, CROP, None, 10, MAXD, MAXR, 0, 5, 8)
    assert r["decision"] == 1 and tuple(r["view"]) == (0, 0) and list(r["update"]) == [-1] * 6
    big = _planted(np.tile([0, 0, 4.0], (3801, 1)), capacity=4000)
    with pytest.raises(ValueError):
        F.track(big, _frame([[0, 0, 4]]), I34, K4, 0.1, ORG, CROP, None, 10, MAXD, MAXR, 0, 5, 8)


# ---- the corridor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("default", {}), ("cross-window", dict(cross_check=True, match_window=(24, 16)))])
def test_fused_chain_equals_the_unfused_chain_on_the_corridor(oracle, name, kw):
    """C1 640x480 frames 0-7, 500 features: with every frame accepted by the map step, the restated fused odometer and map_ref's
    unfused chain agree in decisions, track_source and every count, and in c_T_w to 1e-9 (the project's chained-pose tolerance: the
    device's bracketed product and rigid inverse against numpy's `@` and inv).  cross-window: clones of row 0 in the matcher's
    query set change no cross-check result and carry row 0's window."""
    from openvo_amd import calib
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    Q, roi = calib.stereo_rectify(c.K(), c.dist(), c.K(), c.dist(), (c.w, c.h), c.rect_params()["R"], c.rect_params()["T"])[4:6]
    frames = c.pairs(0, 8)
    cache = {}
    base = dict(max_age=5, max_obs=8, z_min=0.1, capacity=2000, nfeatures=500, pnp_iters=256, pnp_threshold=1.5, pnp_seed=4321, frames=cache)
    a, b = M.MapRefOdometer(oracle, Q, roi, **base, **kw), F.MapFusedRefOdometer(oracle, Q, roi, **base, **kw)
    for k, (L, R) in enumerate(frames):
        ra, rb = a.update(L, R), b.update(L, R)
        assert (ra, a.skip_cause, a.skipped_frames, a.track_source) == (rb, b.skip_cause, b.skipped_frames, b.track_source), k
        assert {n: tuple(int(x) for x in v) for n, v in a.map_counts.items()} == {n: tuple(int(x) for x in v) for n, v in b.map_counts.items()}, k
        assert np.abs(a.c_T_w - b.c_T_w).max() <= 1e-9, (k, np.abs(a.c_T_w - b.c_T_w).max())
    assert b.decisions == [0] * 7 and a.log == b.log
    assert b.map_counts["view"][1] < b.map_counts["view"][0]          # (there WAS padding: not every landmark is in view)
    wa, wb = a.map.download(), b.map.download()
    for n in ("desc", "rdesc", "octave", "obs", "last"):
        assert np.array_equal(wa[n], wb[n]), n
    assert np.abs(wa["xyz"] - wb["xyz"]).max() <= 1e-5
    print("%s: largest |c_T_w fused - unfused| over 8 frames %.3g; map of %d landmarks, last view %s" % (
        name, np.abs(a.c_T_w - b.c_T_w).max(), len(b.map), tuple(b.map_counts["view"])))
