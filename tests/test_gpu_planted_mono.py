"""Planted tests of the monocular pose tail on the device (vo_recover_pose: rp_tail / rs_svd3 in csrc/ransac.hip): scenes from
tests/planted_mono.py that force every vote tie, put inliers on both sides of the parallax gate and on it, give the radix select
equal runs, low-byte and top-byte patterns and every small n_shared, walk every arm of the 3x3 decomposition, cross the
1024-thread stride up to the ABI's 65536 points, and combine the refusals.  The fused finish (k_mono_pose_finish) is met through
mono_pose_pair on frame pairs that leave fewer matches than a solver needs, exactly six and exactly eight.

Every case goes through ctx.recover_pose and is held to mono_pose_ref.recover_pose (the restatement, from E -- not from the
device's pose): integers, votes4, winner, flags and the valid set exactly; z1, z2, depth_b and scale_rel to 1e-12 relative; R and
t to 1e-12 of their unit norm.  scale_rel is held BIT FOR BIT to the numpy lower median of depth_a[q_i] / z1_i over the shared
set with the z1 the device returned.  The module's last test asserts that every regime was reached."""
import numpy as np
import pytest

import mono_pose_ref as ref
import planted_mono as PM
from openvo_amd import _native

pytestmark = pytest.mark.gpu

K4 = list(PM.K4)
SEEN = dict(winners=set(), arms=set(), essentials=set(), select={}, sizes=set(), finish=set())


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 640, 480, 16, 2000)
    yield c
    c.close()


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _rel(a, b, rel=1e-12):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= rel * np.abs(b)))


def _check(ctx, E, p1, p2, mask=None, q=None, t=None, na=None, nb=None, depth_a=None, gate=0.0, K4=K4):
    """one call of the device against the restatement -> (device, restatement); K4: the camera of both (the module's unless given)"""
    got = ctx.recover_pose(E, p1, p2, K4, mask, q, t, na, nb, depth_a, gate)
    r = ref.recover_pose(E, p1, p2, K4, mask, q, t, na, nb, depth_a, gate)
    n = len(p1)
    n_inl = n if mask is None else int(np.count_nonzero(mask))
    for k in ("flags", "winner", "n_depth", "n_shared"):
        assert got[k] == r[k], (k, got[k], r[k])
    assert (got["matches"], got["best_iter"], got["best_count"], got["serial"]) == (n, -1, n_inl, 0)
    assert np.array_equal(got["votes4"], r["votes4"]), (got["votes4"], r["votes4"])
    assert np.array_equal(got["E"], np.asarray(E, np.float64).reshape(3, 3), equal_nan=True)
    assert np.abs(got["R"] - r["R"]).max() <= 1e-12 and np.abs(got["t"] - r["t"]).max() <= 1e-12
    assert np.array_equal(got["depth_b"] != 0, r["depth_b"] != 0)                  # the valid set, as its owners
    if q is None:
        assert np.array_equal(got["depth_b"] != 0, r["valid"])
    for k in ("depth_b", "z1", "z2"):
        assert _rel(got[k], r[k]), k
    if np.isfinite(r["scale_rel"]):
        assert _rel(got["scale_rel"], r["scale_rel"])
    if depth_a is not None and not (got["flags"] & 3):
        d = np.asarray(depth_a, np.float64)[np.arange(n) if q is None else q]
        ratios, _ = PM.actual_ratios(d, got["z1"], r["valid"])
        assert len(ratios) == got["n_shared"]
        want = np.sort(ratios)[(len(ratios) - 1) // 2] if len(ratios) else 0.0
        assert _bits(got["scale_rel"]) == _bits(want), (got["scale_rel"], want)   # (a miss here alone: the device's division)
    return got, r


# ---- a. votes and ties --------------------------------------------------------------------------------------------------------
def test_votes_and_every_tie(ctx):
    for e, (name, E) in enumerate(PM.vote_essentials()):
        tr1, tr2 = PM.traces(E)
        for c, counts4 in enumerate(PM.VOTE_COUNTS):
            p1, p2 = PM.vote_scene(E, counts4, 100 * e + c)
            depth_a = np.full(len(p1), 3.0)
            got, r = _check(ctx, E, p1, p2, depth_a=depth_a)
            assert list(got["votes4"]) == list(counts4), (name, counts4)
            # the rule written out: the largest vote, then the larger trace, then the lower index
            tr = (tr1, tr1, tr2, tr2)
            want = max(range(4), key=lambda k: (counts4[k], tr[k], -k))
            assert got["winner"] == want, (name, counts4, got["winner"], want)
            if counts4 == (5, 5, 0, 0):
                assert want == 0
            elif counts4 == (0, 0, 5, 5):
                assert want == 2
            elif counts4 == (4, 5, 5, 5):
                assert want in (1, 2) and counts4[want] == 5
            elif sum(counts4) == 1:
                assert want == counts4.index(1)
            if any(counts4):
                assert got["n_depth"] == counts4[want] == got["n_shared"] and got["scale_rel"] > 0
            else:
                assert got["n_depth"] == 0 and got["scale_rel"] == 0.0 and got["n_shared"] == 0 and not got["depth_b"].any()
            SEEN["winners"].add(got["winner"])
            SEEN["arms"] |= PM.tie_arms(counts4, tr1, tr2)


# ---- b. the gate --------------------------------------------------------------------------------------------------------------
def test_parallax_gate_on_both_sides_and_on_the_value(ctx):
    s = PM.gate_scene()
    E, p1, p2 = s["E"], s["p1"], s["p2"]
    depth_a = np.full(64, 2.0)
    first, r0 = _check(ctx, E, p1, p2, depth_a=depth_a, gate=0.0)
    assert first["n_depth"] == 64
    near, _ = _check(ctx, E, p1, p2, depth_a=depth_a, gate=PM.GATE)
    valid = near["depth_b"] != 0
    assert valid[56:60].all() and not valid[60:].any()                  # within 1e-9 relative above | below the gate
    assert near["n_depth"] == int(valid.sum()) and 4 < near["n_depth"] < 60
    # a gate that IS one inlier's sin2 (restated from the device's own pose of the first call): >= keeps the inlier
    sin2 = PM.sin2_of(first["R"], first["t"], p1, p2)
    for k in (3, 30, 57, 62):
        on = ctx.recover_pose(E, p1, p2, K4, depth_a=depth_a, min_parallax_sin2=float(sin2[k]))
        v = on["depth_b"] != 0
        assert v[k], k
        assert np.array_equal(v, sin2 >= sin2[k]) and on["n_depth"] == on["n_shared"] == int((sin2 >= sin2[k]).sum())
        assert np.array_equal(on["R"], first["R"]) and np.array_equal(on["z1"], first["z1"])
    above, _ = _check(ctx, E, p1, p2, depth_a=depth_a, gate=float(sin2.max()) * 1.5)
    assert above["n_depth"] == 0 and above["n_shared"] == 0 and above["scale_rel"] == 0.0 and not above["depth_b"].any()
    assert above["flags"] == 0 and np.array_equal(above["z1"], first["z1"])     # (the inliers' depths do not pass the gate's way)


# ---- c. the select ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_scene(ctx):
    E = PM.essential(1)
    p1, p2 = PM.plant_votes(E, (PM.SELECT_N, 0, 0, 0), np.random.default_rng(41))
    first = ctx.recover_pose(E, p1, p2, K4)
    assert first["n_depth"] == PM.SELECT_N and first["winner"] == 0
    return E, p1, p2, first["z1"].copy()


@pytest.mark.parametrize("case", PM.SELECT_CASES)
def test_select_of_the_lower_median(ctx, select_scene, case):
    E, p1, p2, z1 = select_scene
    d, shared = PM.select_depths(case, z1)
    got, r = _check(ctx, E, p1, p2, depth_a=d)
    assert np.array_equal(got["z1"], z1)
    ratios, sh = PM.actual_ratios(d, z1)
    n_shared = int(shared.sum())
    assert got["n_shared"] == n_shared == len(ratios) and np.array_equal(sh, shared)
    want = np.sort(ratios)[(n_shared - 1) // 2]
    print("%s: n_shared %d, rank %d, median %r (0x%016x)" % (case, n_shared, (n_shared - 1) // 2, float(want), _bits(want)))
    assert _bits(got["scale_rel"]) == _bits(want)
    SEEN["select"][case] = got["n_shared"]


# ---- d. the arms of the decomposition -----------------------------------------------------------------------------------------
def _plant_40(E, rng):
    """40 inliers for the restatement's own candidates of E, ten for each candidate that has points in front of both cameras"""
    counts, total = [0, 0, 0, 0], 0
    while total < 40:
        grown = False
        for c in range(4):
            trial = [0, 0, 0, 0]
            trial[c] = 1
            try:
                PM.plant_votes(E, trial, np.random.default_rng(1))
            except RuntimeError:
                continue
            counts[c] += 10
            total += 10
            grown = True
            if total == 40:
                break
        assert grown
    return PM.plant_votes(E, counts, rng)


def test_every_arm_of_the_decomposition(ctx):
    good = PM.vote_scene(PM.essential(1), (40, 0, 0, 0), 5)
    for k, (name, E, kind) in enumerate(PM.essentials()):
        if kind == "refused":
            nb = 57
            q, t = np.arange(40, dtype=np.int32), np.arange(40, dtype=np.int32) + 17
            got, r = _check(ctx, E, good[0], good[1], None, q, t, 40, nb, np.full(40, 2.0))
            assert got["flags"] == 1 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and not got["votes4"].any()
            assert not got["z1"].any() and not got["z2"].any() and not got["depth_b"].any() and len(got["depth_b"]) == nb
            assert (got["winner"], got["n_depth"], got["n_shared"], got["scale_rel"]) == (0, 0, 0, 0.0)
            assert np.array_equal(got["E"], E, equal_nan=True)
        else:
            p1, p2 = _plant_40(E, np.random.default_rng([51, k]))
            got, r = _check(ctx, E, p1, p2, depth_a=np.full(40, 2.0))
            assert got["flags"] == 0 and got["votes4"].sum() == 40 and got["n_depth"] == got["votes4"].max()
            assert np.abs(got["R"] @ got["R"].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(got["R"]) - 1.0) <= 1e-12
            U, w, _ = np.linalg.svd(E)
            if kind == "full":
                assert min(np.abs(got["t"] - U[:, 2]).max(), np.abs(got["t"] + U[:, 2]).max()) <= 1e-12, name
            else:
                assert abs(got["t"] @ U[:, 0]) <= 1e-12 and abs(np.linalg.norm(got["t"]) - 1.0) <= 1e-12, name
        SEEN["essentials"].add(name)


# ---- e. strides and sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PM.STRIDE_SIZES)
def test_block_stride_sizes(ctx, n):
    E = PM.essential(1)
    p1, p2 = PM.stride_scene(n)
    rng = np.random.default_rng([61, n])
    depth_a = np.where(rng.random(n) < 0.1, 0.0, rng.uniform(1.0, 9.0, n))
    full, _ = _check(ctx, E, p1, p2, depth_a=depth_a)
    k = n // 8
    assert list(full["votes4"]) == [n - 3 * k, k, k, k] and full["n_depth"] == n - 3 * k and full["winner"] == 0
    mask = PM.last_of_word_mask(n)
    sparse, _ = _check(ctx, E, p1, p2, mask=mask, depth_a=depth_a)
    assert sparse["best_count"] == n // 64 and sparse["votes4"].sum() == n // 64
    assert not sparse["z1"][mask == 0].any() and np.array_equal(sparse["z1"][mask != 0], full["z1"][mask != 0])
    SEEN["sizes"].add(n)


def test_keypoint_frames_larger_than_the_correspondences(ctx):
    E = PM.essential(1)
    n, na, nb = 65, 70, 100000
    p1, p2 = PM.plant_votes(E, (50, 5, 5, 5), np.random.default_rng(71))
    rng = np.random.default_rng(72)
    q, t = rng.permutation(na)[:n].astype(np.int32), rng.permutation(nb)[:n].astype(np.int32)
    t[0], t[64] = nb - 1, 0
    depth_a = rng.uniform(1.0, 5.0, na)
    # twice: what the first call left in the scratch must not show in the second
    for _ in range(2):
        got, r = _check(ctx, E, p1, p2, None, q, t, na, nb, depth_a)
        named = np.zeros(nb, bool)
        named[t[r["valid"]]] = True
        assert got["n_depth"] == 50 and len(got["depth_b"]) == nb and np.array_equal(got["depth_b"] != 0, named)
        t = t[::-1].copy()
        p1, p2, q = p1[::-1].copy(), p2[::-1].copy(), q[::-1].copy()


def test_one_keypoint_named_from_different_waves_and_trips(ctx):
    E = PM.essential(1)
    n = 2100
    p1, p2 = PM.plant_votes(E, (n, 0, 0, 0), np.random.default_rng(81))
    q = np.arange(n, dtype=np.int32)
    t = np.arange(n, dtype=np.int32)
    t[5 + 1024] = t[5 + 2048] = 5                  # three loop trips of one thread
    t[7 + 1024] = t[7 + 2048] = 7                  # ... the lowest of them no inlier
    t[200] = t[1500] = t[70]                       # different waves
    mask = np.ones(n, np.uint8)
    mask[7] = 0
    got, r = _check(ctx, E, p1, p2, mask, q, t, n, n, np.full(n, 2.0))
    assert got["n_depth"] == n - 1
    assert got["depth_b"][5] == got["z2"][5] != 0 and got["depth_b"][7] == got["z2"][7 + 1024] != 0
    assert got["depth_b"][70] == got["z2"][70] != 0
    for gone in (5 + 1024, 5 + 2048, 7 + 1024, 7 + 2048, 200, 1500):
        assert got["depth_b"][gone] == 0.0


# ---- f. refusals together -----------------------------------------------------------------------------------------------------
def test_refusals_together_and_the_call_after(ctx):
    E = PM.essential(1)
    n = 100
    p1, p2 = PM.plant_votes(E, (70, 10, 10, 10), np.random.default_rng(91))
    q, t = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy()
    depth_a = np.linspace(1.0, 4.0, n)

    def good():
        g, _ = _check(ctx, E, p1, p2, None, q, t, n, n, depth_a, PM.GATE)
        assert g["flags"] == 0 and g["n_depth"] > 0 and g["n_shared"] > 0
        return g

    def same(a, b):
        assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]

    before = good()
    # an index out of range with no depths: bits 1 and 2 together, the call is refused
    for bad_q, bad_t in ((None, (17, n)), ((3, -1), None), ((99, n), (0, -5))):
        qq, tt = q.copy(), t.copy()
        if bad_q:
            qq[bad_q[0]] = bad_q[1]
        if bad_t:
            tt[bad_t[0]] = bad_t[1]
        with pytest.raises(_native.VoError) as e:
            ctx.recover_pose(E, p1, p2, K4, None, qq, tt, n, n, None, PM.GATE)
        assert e.value.code == -3
        assert ref.recover_pose(E, p1, p2, K4, None, qq, tt, n, n, None, PM.GATE)["flags"] == 6
        same(good(), before)
    # no inlier, depths given: bit 0 alone
    g, _ = _check(ctx, E, p1, p2, np.zeros(n, np.uint8), q, t, n, n, depth_a, PM.GATE)
    assert g["flags"] == 1 and g["best_count"] == 0 and np.array_equal(g["R"], np.eye(3))
    assert not g["t"].any() and not g["z1"].any() and not g["z2"].any() and not g["depth_b"].any() and not g["votes4"].any()
    g, _ = _check(ctx, E, p1, p2, np.zeros(n, np.uint8), q, t, n, n, None, PM.GATE)
    assert g["flags"] == 5
    same(good(), before)
    # arguments: VO_E_ARG (-1) for a bad argument, VO_E_CAP (-4) for n outside 1 .. 65536
    for kw, code in ((dict(gate=-1e-300), -1), (dict(gate=float("nan")), -1), (dict(k4=[0.0, 400.0, 320.0, 240.0]), -1),
                     (dict(k4=[-400.0, 400.0, 320.0, 240.0]), -1), (dict(n=0), -4), (dict(n=65537), -4)):
        m = kw.get("n", n)
        a, b = (p1, p2) if m == n else (np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32))
        with pytest.raises(_native.VoError) as e:
            ctx.recover_pose(E, a, b, kw.get("k4", K4), None, None, None, None, None, None, kw.get("gate", PM.GATE))
        assert e.value.code == code, (kw, e.value.code)
        same(good(), before)


# ---- g. the fused finish ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PM.FINISH_SEEDS))
def test_fused_finish_below_at_and_above_the_minimum(ctx, name):
    seed, M = PM.FINISH_SEEDS[name]
    xy = []
    for slot, frame in zip((20, 21), PM.finish_frames(seed)):
        ctx.upload_mono(slot, frame)
        assert ctx.orb_slot_count(slot, 2000, 0) >= 3
        xy.append(ctx.download_keypoints_xy(slot))
    na, nb = len(xy[0]), len(xy[1])
    args = (PM.FINISH_RATIO, K4, 256, 1.0, 4321)
    for solver in (5, 8):
        got = ctx.mono_pose_pair(20, 21, *args, solver, False, prev_serial=0, min_parallax_sin2=0.0)
        live = M >= (6 if solver == 5 else 8)
        print("%s, solver %d: %d keypoints, %d matches, best_count %d, flags %d" % (name, solver, na, got["matches"], got["best_count"], got["flags"]))
        assert got["matches"] == M                                     # (as the CPU oracle counts them)
        depth, serial = ctx.download_mono_depth(21)
        assert serial == got["serial"] != 0 and len(depth) == nb           # stamped whatever became of the step
        if not live:
            assert got["best_count"] == 0 and got["flags"] == 5 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any()
            assert (got["winner"], got["n_depth"], got["n_shared"], got["scale_rel"]) == (0, 0, 0, 0.0)
            assert not got["votes4"].any() and not depth.any()
            continue
        comp = ctx.mono_pair(20, 21, *args, want_matches=True, solver=solver)
        assert (comp["matches"], comp["best_iter"], comp["best_count"]) == (got["matches"], got["best_iter"], got["best_count"])
        assert np.array_equal(got["E"], comp["E"]) and len(comp["q"]) == M
        p1, p2 = xy[0][comp["q"]], xy[1][comp["t"]]
        rp = ctx.recover_pose(comp["E"], p1, p2, K4, comp["mask"], comp["q"], comp["t"], na, nb, None, 0.0)
        for k in ("winner", "n_depth", "n_shared", "flags", "scale_rel"):
            assert got[k] == rp[k], (k, got[k], rp[k])
        for k in ("votes4", "R", "t"):
            assert np.array_equal(got[k], rp[k]), k
        assert np.array_equal(depth, rp["depth_b"])
    SEEN["finish"].add(name)


# ---- the regimes reached ------------------------------------------------------------------------------------------------------
def test_every_regime_was_reached():
    assert SEEN["winners"] == {0, 1, 2, 3}, SEEN["winners"]
    assert SEEN["arms"] == PM.ALL_TIE_ARMS, SEEN["arms"]
    assert SEEN["essentials"] == {name for name, _, _ in PM.essentials()}
    want = {case: int(PM.select_targets(case)[1].sum()) for case in PM.SELECT_CASES}
    assert SEEN["select"] == want and {want["shared_%d" % k] for k in (1, 2, 3, 255, 256, 257)} == {1, 2, 3, 255, 256, 257}
    assert SEEN["sizes"] == set(PM.STRIDE_SIZES) and SEEN["finish"] == set(PM.FINISH_SEEDS)
