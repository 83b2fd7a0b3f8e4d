"""The numpy restatement of the PnP step's local-optimisation rounds (tests/pnp_lo_ref.py) held to what the rounds must do, the
planted cases of the GPU tests (tests/planted_pnp_lo.py) held to their admission condition and their regimes, the figures of
DESIGN 4g regenerated, and the odometer's host logic on a scripted context.  CPU only; the GPU kernel is then held to the
restatement (tests/test_gpu_planted_pnp_lo.py)."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_lo_ref as PL                    # noqa: E402
import pnp_refine_ref as PR                # noqa: E402
import planted_pnp as PP                   # noqa: E402
import planted_pnp_lo as PLO               # noqa: E402
import sparse_stereo_ref as S              # noqa: E402
from planted_pnp import PnpCase            # noqa: E402

SEEDS = (4321, 1, 2, 3, 4, 5, 6, 7)
THR = 1.5


def _pnp_scene(n, seed, outlier_frac=0.3, noise=0.3):
    """the scene generator of tests/test_pnp_refine_ref.py (copied: a test file is not imported)"""
    rng = np.random.default_rng(seed)
    f, cx, cy = 718.856, 640.0, 360.0
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)], 1)
    r = np.array([0.01, -0.03, 0.005])
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.05, -0.02, -0.3])
    Xc = X @ R.T + t
    uv = np.stack([f * Xc[:, 0] / Xc[:, 2] + cx, f * Xc[:, 1] / Xc[:, 2] + cy], 1) + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, int(n * outlier_frac), replace=False)
    uv[out] += rng.uniform(-60, 60, size=(len(out), 2))
    return X.astype(np.float32), uv.astype(np.float32), [f, f, cx, cy], R, t, out


def _noiseless(n=80, seed=3):
    """as tests/test_pnp_refine_ref.py"""
    rng = np.random.default_rng(seed)
    f, cx, cy = 718.856, 640.0, 360.0
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)], 1).astype(np.float32)
    R = PR.exp_so3(np.array([0.02, -0.05, 0.01]))
    t = np.array([0.1, -0.05, -0.4])
    Xc = X.astype(np.float64) @ R.T + t
    uv = np.stack([f * Xc[:, 0] / Xc[:, 2] + cx, f * Xc[:, 1] / Xc[:, 2] + cy], 1).astype(np.float32)
    return X, uv, [f, f, cx, cy], R, t


# ---- 1. one round is today's refit -------------------------------------------------------------------------------------------------
def test_the_float32_test_is_the_oracles(oracle):
    """select() under the winner's own P gives the oracle's mask: the restated test is the scoring kernels' test"""
    for n, s in ((200, 0), (60, 1), (1000, 2)):
        X, uv, K4, *_ = _pnp_scene(n, 1000 * n + s)
        r = oracle.ransac_pnp(X, uv, K4, 64, THR, 4321)
        assert np.array_equal(PL.select(PL.form_P(r["Rt"], K4), X, uv, THR), r["mask"]), (n, s)


@pytest.mark.parametrize("steps", [1, 3, 5])
def test_one_round_is_the_plain_refit_bit_for_bit(oracle, steps):
    for n, s in ((200, 0), (30, 1), (500, 2)):
        X, uv, K4, *_ = _pnp_scene(n, 1000 * n + s)
        r = oracle.ransac_pnp(X, uv, K4, 64, THR, 4321)
        Rt0 = np.asarray(r["Rt"], np.float64).reshape(3, 4)
        want, status, k = PR.refine(Rt0, X, uv, K4, r["mask"], steps)
        Rt, S, st, nsteps, c = PL.lo(Rt0, r["mask"], X, uv, K4, THR, steps, 1)
        assert (status, k) == (0, steps) and (st, nsteps, c) == (0, steps, 1)
        assert np.array_equal(Rt, want)
        assert np.array_equal(S, PL.select(PL.form_P(want, K4), X, uv, THR))
        # the rounds are prefixes of one another: round r does not know how many follow
        tr = []
        PL.lo(Rt0, r["mask"], X, uv, K4, THR, steps, 3, trace=tr)
        assert np.array_equal(tr[0][1], S)


def test_arguments_outside_the_definition_are_refused():
    X, uv, K4, R, t = _noiseless(20)
    start = np.hstack([R, t[:, None]])
    for steps, rounds in ((0, 1), (21, 1), (3, 0), (3, 9)):
        with pytest.raises(ValueError):
            PL.lo(start, np.ones(20, np.uint8), X, uv, K4, THR, steps, rounds)


# ---- 2. a round that cannot run ----------------------------------------------------------------------------------------------------
def test_a_round_that_cannot_run_leaves_the_round_before(oracle):
    # (a) the planted support that falls below 6: round 1 completes with 5 points, round 2 is not attempted, whatever R asks for
    c = PLO.case("support_crosses_6")
    m = c.model(oracle)
    assert m["best_count"] == 6
    one = PL.lo(m["Rt"], m["mask"], m["X"], m["uv"], c.K4, PP.THR, 3, 1)
    for rounds in (2, 3, 8):
        Rt, Sm, status, nsteps, done = PL.lo(m["Rt"], m["mask"], m["X"], m["uv"], c.K4, PP.THR, 3, rounds)
        assert (status, nsteps, done, int(Sm.sum())) == (0, 3, 1, 5)
        assert np.array_equal(Rt, one[0]) and np.array_equal(Sm, one[1])
    # (b) the degenerate sets of tests/test_pnp_refine_ref.py: round 1 fails, the result is the input and the status is the refit's
    X, uv, K4, R, t = _noiseless(20)
    start = np.hstack([R, t[:, None]])
    Xs, uvs = np.repeat(X[:1], 8, 0), np.repeat(uv[:1], 8, 0)                # one point eight times: J^T J has rank 2
    Rt, Sm, status, nsteps, done = PL.lo(start, np.ones(8, np.uint8), Xs, uvs, K4, THR, 5, 3)
    assert (status, nsteps, done) == (-1, 0, 0) and np.array_equal(Rt, start) and Sm.all()
    Xz = X[:8].copy()                                                        # a point in the camera's plane: non-finite sums
    Xz[0] = (np.linalg.inv(R) @ (np.array([1.0, 1.0, 0.0]) - t)).astype(np.float32)
    start0 = start.copy()
    start0[2, 3] -= float(start0[2, :3] @ Xz[0].astype(np.float64) + start0[2, 3])
    Rt, Sm, status, nsteps, done = PL.lo(start0, np.ones(8, np.uint8), Xz, uv[:8], K4, THR, 5, 2)
    assert (status, nsteps, done) == (-1, 0, 0) and np.array_equal(Rt, start0)
    S5 = np.r_[np.ones(5, np.uint8), np.zeros(15, np.uint8)]                 # five points: not attempted
    Rt, Sm, status, nsteps, done = PL.lo(start, S5, X, uv, K4, THR, 5, 8)
    assert (status, nsteps, done) == (1, 0, 0) and np.array_equal(Rt, start) and np.array_equal(Sm, S5)
    # (c) a LATER round cannot run: round 1 runs on all 20 points; under a threshold of 1e-9 px nothing is re-selected, so round 2
    # has no set -- rounds 2 .. 4 are not attempted, the status stays 0 and the result is round 1's
    Rt1, S1, status, nsteps, done = PL.lo(start, np.ones(20, np.uint8), X, uv, K4, 1e-9, 3, 4)
    assert (status, done, nsteps) == (0, 1, 3) and int(S1.sum()) < 6
    assert np.array_equal(Rt1, PR.refine(start, X, uv, K4, np.ones(20, np.uint8), 3)[0])


# ---- the planted cases of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rounds,steps", PLO.ALL, ids=["%s-R%d-s%d" % a for a in PLO.ALL])
def test_planted_cases_are_admitted(oracle, name, rounds, steps):
    """THE ADMISSION CONDITION: sequential, thread-strided and longdouble sums give the same float32 P and the same set in every
    round (and no point within 1e-4 of the threshold).  A case that fails it is replaced, not kept."""
    lm = PLO.lo_model(PLO.case(name), oracle, rounds, steps)
    sup = [int(Sm.sum()) for _, Sm in lm["trace"]]
    print("%s R%d x %d: winner %d -> %s, rounds %d, nearest point %.2g from the threshold" % (
        name, rounds, steps, PLO.case(name).model(oracle)["best_count"], sup, lm["rounds"], lm["margin"]))
    assert PLO.admitted(lm)
    d = max(float(np.abs(lm["Rt"] - lm["Rt_strided"]).max()), float(np.abs(lm["Rt"] - lm["Rt_ld"]).max()))
    assert d < 1e-11, d                      # (the bar of the GPU test is 1e-9: the order of the sums uses a hundredth of it)


def test_planted_cases_reach_their_regimes(oracle):
    n = {c.name: c.model(oracle)["n"] for c, _ in PLO.CASES}
    assert [n[k] for k in ("n6_all_planted", "n7_six_grow_to_seven", "n255", "n256", "n257", "n603")] == [6, 7, 255, 256, 257, 603]
    grew = shrank = 0
    for c, runs in PLO.CASES:
        m = c.model(oracle)
        assert m["best_count"] >= 6 and m["status"] == 0, c.name
        for rounds, steps in runs:
            lm = PLO.lo_model(c, oracle, rounds, steps)
            sup = [m["best_count"]] + [int(Sm.sum()) for _, Sm in lm["trace"]]
            grew += any(b > a for a, b in zip(sup, sup[1:]))
            shrank += any(b < a for a, b in zip(sup, sup[1:]))
            # a set CHANGES, it is not only counted: some point enters or leaves in some round of the larger cases
            if m["n"] >= 255:
                assert any(not np.array_equal(a, b) for a, b in zip([m["mask"]] + [Sm for _, Sm in lm["trace"]], [Sm for _, Sm in lm["trace"]]))
            if c.name != "support_crosses_6":
                assert lm["rounds"] == rounds, (c.name, rounds, steps)
    assert grew >= 10 and shrank >= 2, (grew, shrank)
    m6 = PLO.case("n6_all_planted").model(oracle)
    assert m6["best_count"] == 6 and m6["mask"].all()
    m7 = PLO.case("n7_six_grow_to_seven").model(oracle)
    assert m7["best_count"] == 6 and PLO.lo_model(PLO.case("n7_six_grow_to_seven"), oracle, 1, 3)["support"] == 7
    second = PLO.case("inliers300_second_pass_on")
    assert not second.model(oracle)["mask"][:256].any()
    for _, Sm in PLO.lo_model(second, oracle, 3, 3)["trace"]:
        assert not Sm[:256].any() and Sm[256:].sum() >= 100           # the first trip of the strided loop counts nothing
    cross = PLO.lo_model(PLO.case("support_crosses_6"), oracle, 8, 5)
    assert (cross["rounds"], cross["support"], cross["status"], cross["steps"]) == (1, 5, 0, 5)


def test_the_small_scenes_can_be_found_again(oracle):
    """the loops that found N6_SCENE, N7_SCENE and CROSS_SCENE: the first scene seed that reaches the regime"""
    def first(make, hit):
        for scene in range(64):
            c = make(scene)
            if hit(c, c.model(oracle)):
                return scene
    assert first(lambda s: PnpCase("x", 9, 6, n_in=6, noise=0.5, refine=3, scene=s), lambda c, m: m["best_count"] == 6) == PLO.N6_SCENE
    assert first(lambda s: PnpCase("x", 10, 7, n_in=7, noise=0.8, refine=3, scene=s),
                 lambda c, m: m["best_count"] == 6 and PLO.lo_model(c, oracle, 1, 3)["support"] == 7) == PLO.N7_SCENE
    assert first(lambda s: PLO.RingCase("x", 15, 12, n_in=8, refine=3, scene=s, ring=1.35),
                 lambda c, m: m["best_count"] >= 6 and PLO.lo_model(c, oracle, 2, 3)["rounds"] < 2) == PLO.CROSS_SCENE


def test_planted_map_cases_reach_their_regimes(oracle):
    """the two frames of test_gpu_planted_pnp_lo.py::test_track_map_lo, on the restated map view"""
    import test_gpu_planted_pnp_lo as TL
    _, f, view, _ = TL.map_case("accepted_3_rounds")
    m, lm = TL.map_lo_model(oracle, view, f)
    sup = [m["best_count"]] + [int(Sm.sum()) for _, Sm in lm["trace"]]
    print("accepted_3_rounds: n %d, supports %s, nearest point %.2g from the threshold" % (m["n"], sup, lm["margin"]))
    assert PLO.admitted(lm) and lm["rounds"] == 3 and lm["status"] == 0 and len(set(sup)) > 1 and m["best_count"] >= 10
    _, f, view, _ = TL.map_case("no_round_can_run")
    m, lm = TL.map_lo_model(oracle, view, f)
    print("no_round_can_run: n %d, winner %d" % (m["n"], m["best_count"]))
    assert PLO.admitted(lm) and 4 <= m["best_count"] < 6 and m["M"] >= 4 and m["n"] >= 4
    assert (lm["rounds"], lm["status"], lm["steps"], lm["support"]) == (0, 1, 0, m["best_count"]) and np.array_equal(lm["mask"], m["mask"])


# ---- 3. the synthetic scenes -------------------------------------------------------------------------------------------------------
SCENES = [(200, .3, .3), (500, .3, .3), (60, .2, .5), (1000, .5, .3), (30, .3, .3)]


@pytest.fixture(scope="module")
def scenes(oracle):
    """20 scenes x 8 seeds, 64 hypotheses: today's refit (3 steps) and 3 rounds x 3 steps -> rows of
    (scene, seed, winner's count, |t - truth| refit, |t - truth| LO, support, the final set)"""
    rows = []
    for n, frac, noise in SCENES:
        for s in range(4):
            X, uv, K4, R, t, _ = _pnp_scene(n, 1000 * n + s, frac, noise)
            for seed in SEEDS:
                r = oracle.ransac_pnp(X, uv, K4, 64, THR, seed)
                Rt0 = np.asarray(r["Rt"], np.float64).reshape(3, 4)
                tr = []
                Rt3, S3, status, _, done = PL.lo(Rt0, r["mask"], X, uv, K4, THR, 3, 3, trace=tr)
                Rt1 = PR.refine(Rt0, X, uv, K4, r["mask"], 3)[0]
                rows.append(((n, s), seed, int(r["best_count"]), float(np.linalg.norm(Rt1[:, 3] - t)), float(np.linalg.norm(Rt3[:, 3] - t)),
                             int(S3.sum()), S3.tobytes(), status, done))
    return rows


def test_rounds_on_20_scenes_by_8_seeds(scenes):
    """With 64 hypotheses, 3 rounds x 3 steps against today's 3 steps: the spread of the translation error over the RANSAC seeds
    (std and max) is lower or equal in all 20 scenes; the support never falls below the winner's count; the final set is THE SAME
    SET for all 8 seeds in at least 19 scenes."""
    assert len(scenes) == 160 and all(r[7] == 0 and r[8] == 3 for r in scenes)
    assert all(r[5] >= r[2] for r in scenes), [r[:3] + (r[5],) for r in scenes if r[5] < r[2]]
    std_ok = max_ok = mean_ok = same = 0
    print("scene          refit 3: mean / max / std        3 x 3: mean / max / std     sets")
    for key in sorted({r[0] for r in scenes}):
        rr = [r for r in scenes if r[0] == key]
        e1, e3 = np.array([r[3] for r in rr]), np.array([r[4] for r in rr])
        sets = len({r[6] for r in rr})
        print("n%-5d s%d     %.5f / %.5f / %.5f     %.5f / %.5f / %.5f     %d" % (key[0], key[1], e1.mean(), e1.max(), e1.std(), e3.mean(), e3.max(), e3.std(), sets))
        std_ok += e3.std() <= e1.std()
        max_ok += e3.max() <= e1.max()
        mean_ok += e3.mean() <= e1.mean()
        same += sets == 1
    print("std lower or equal in %d / 20, max in %d / 20, mean in %d / 20; one final set for all seeds in %d / 20" % (std_ok, max_ok, mean_ok, same))
    assert std_ok == 20 and max_ok == 20
    assert same >= 19


# ---- 4. the corridor ---------------------------------------------------------------------------------------------------------------
LoRefOdometer = PL.LoRefOdometer


@pytest.fixture(scope="module")
def corridor(oracle):
    """end-point error (metres) after 12 pairs, per RANSAC seed, of refine 0 / refine 3 / 2 x 3 / 3 x 3 on four rows"""
    from openvo_amd import calib
    from openvo_amd.synth import Corridor
    out = {}
    for scene, first in (("C1", 0), ("C2", 20)):
        c = Corridor(scene)
        Q, roi = calib.stereo_rectify(c.K(), c.dist(), c.K(), c.dist(), (c.w, c.h), c.rect_params()["R"], c.rect_params()["T"])[4:6]
        frames = c.pairs(first, 13)
        gt = np.linalg.inv(type(c).gt_pose(first)) @ type(c).gt_pose(first + 12)
        cache = {}
        for iters in (256, 64):
            memo = {}
            table = {}
            for name, refine, rounds in (("refine 0", 0, 0), ("refine 3", 3, 0), ("2 x 3", 3, 2), ("3 x 3", 3, 3)):
                errs = []
                for seed in SEEDS:
                    odo = LoRefOdometer(oracle, Q, roi, nfeatures=500, pnp_iters=iters, pnp_threshold=THR, pnp_seed=seed, frames=cache, refine=refine,
                                        rounds=rounds, memo=memo)
                    for L, R in frames:
                        odo.update(L, R)
                    errs.append(float(np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3])))
                table[name] = errs
            out[(scene, first, iters)] = table
    return out


def test_corridor_table(corridor):
    """The table of DESIGN 4g.  Asserted: C1 frames 0 - 12 with 256 hypotheses, 3 rounds x 3 steps beat refine 3 for every one of
    the 8 seeds.  The C2 rows are printed, not asserted: they are mixed (DESIGN says so)."""
    for (scene, first, iters), table in corridor.items():
        print("%s %d-%d, %d hyp.: mean / max / std over the seeds %s" % (scene, first, first + 12, iters, SEEDS))
        for name, errs in table.items():
            e = np.array(errs)
            print("    %-9s %.4f / %.4f / %.4f    %s" % (name, e.mean(), e.max(), e.std(), " ".join("%.4f" % v for v in errs)))
        better = sum(a < b for a, b in zip(table["3 x 3"], table["refine 3"]))
        print("    3 x 3 beats refine 3 for %d of 8 seeds, mean ratio %.2f" % (better, np.mean(table["3 x 3"]) / np.mean(table["refine 3"])))
    t = corridor[("C1", 0, 256)]
    assert all(a < b for a, b in zip(t["3 x 3"], t["refine 3"])), (t["3 x 3"], t["refine 3"])
    assert all(a < b for a, b in zip(t["refine 3"], t["refine 0"]))           # (DESIGN 4g's own table: 8 of 8)


# ---- 5. host logic on a scripted context -------------------------------------------------------------------------------------------
from openvo_amd import StereoOdometer, _native      # noqa: E402
from openvo_amd.stereo_odometer import LoopCheck, LoRounds      # noqa: E402


def test_abi_and_binding():
    import ctypes
    _native.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ("vo_pnp_pair_lo", "vo_pnp_pair_begin_lo", "vo_pnp_pair_end_lo", "vo_track_map_lo"):
        assert hasattr(L, name) and name in _native.SYMBOLS, name
    for name in ("pnp_pair_lo", "pnp_pair_begin_lo", "pnp_pair_end_lo", "track_map_lo"):
        assert callable(getattr(_native.Context, name, None)), name
    lib, ci, vp = _native.lib(), ctypes.c_int, ctypes.c_void_p
    assert list(lib.vo_pnp_pair_lo.argtypes) == list(lib.vo_pnp_pair.argtypes) + [ci, vp]
    assert list(lib.vo_pnp_pair_begin_lo.argtypes) == list(lib.vo_pnp_pair_begin.argtypes)[:-1] + [ci, vp]
    assert list(lib.vo_pnp_pair_end_lo.argtypes) == list(lib.vo_pnp_pair_end.argtypes) + [vp]
    assert list(lib.vo_track_map_lo.argtypes) == list(lib.vo_track_map.argtypes) + [ci]
    for bad in (-1, 9, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            _native.Context.lo_rounds_arg(bad, 3)
    with pytest.raises(ValueError):
        _native.Context.lo_rounds_arg(1, 0)
    assert _native.Context.lo_rounds_arg(0, 0) == 0 and _native.Context.lo_rounds_arg(np.int64(8), 1) == 8


def test_constructor_validates_pnp_lo_rounds():
    assert StereoOdometer(None, pose_method="pnp").pnp_lo_rounds == 0
    assert "pnp_lo_rounds" not in StereoOdometer(None, pose_method="pnp", pnp_refine=3).__dict__
    assert StereoOdometer(None, pose_method="pnp", pnp_refine=3, pnp_lo_rounds=np.int64(8)).pnp_lo_rounds == 8
    for bad in (-1, 9, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            StereoOdometer(None, pose_method="pnp", pnp_refine=3, pnp_lo_rounds=bad)
    with pytest.raises(ValueError):
        StereoOdometer(None, pose_method="pnp", pnp_lo_rounds=2)                        # rounds without refit steps
    with pytest.raises(ValueError):
        StereoOdometer(None, pnp_refine=3, pnp_lo_rounds=2)                             # rounds without the PnP mode
    assert StereoOdometer(None, pnp_lo_rounds=0).pnp_lo_rounds == 0


class _Stereo:
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 500.0], [0, 0, 2.0, 0]])

    def slot_key(self, s):
        return (s, 0)


def _bound(fn, *a, **kw):
    b = inspect.signature(getattr(_native.Context, fn)).bind(None, *a, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k != "self"}


class _Ctx:
    """stands in for _native.Context: every call is logged by name and bound against the real method's signature"""
    NAMES = ("pnp_pair", "pnp_pair_window", "pnp_pair_begin", "pnp_pair_begin_window", "pnp_pair_end", "pnp_pair_lo", "pnp_pair_begin_lo",
             "pnp_pair_end_lo", "map_track", "track_map_lo")

    def __init__(self, rec):
        self.rec, self.log = rec, []

    def __getattr__(self, name):
        if name not in self.NAMES:
            raise AttributeError(name)

        def call(*a, **kw):
            self.log.append((name, _bound(name, *a, **kw)))
            if "begin" in name:
                return 40 + len(self.log)
            rec = dict(self.rec)
            if not name.endswith("_lo"):
                rec.pop("lo_rounds", None), rec.pop("lo_support", None)
            return rec
        return call

    @staticmethod
    def rodrigues(R):
        return _native.Context.rodrigues(R)


def _rt(angle, dist):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, dist], [0, 1, 0, 0], [-s, 0, c, 0]], np.float64)


WIN, REF = _rt(0.01, 0.20), _rt(0.02, 0.25)


def _rec(best_count=30, status=0, rounds=3, support=44, **kw):
    return dict(dict(matches=50, n=40, best_iter=7, best_count=best_count, flags=0, Rt=WIN, Rt_refined=REF, refine_status=status,
                     refine_steps=3 * rounds if status == 0 else 0, lo_rounds=rounds if status == 0 else 0, lo_support=support), **kw)


def _odo(rec, **kw):
    od = StereoOdometer(None, pose_method="pnp", **kw)
    od.stereo, od._ctx, od.skip_cause = _Stereo(), _Ctx(rec), "init"
    return od


def test_rounds_0_makes_todays_calls_and_no_others():
    K4 = (500.0, 500.0, 320.0, 240.0)
    od = _odo(_rec(), pnp_refine=3)
    params = od._pose_params()
    assert params == ("pnp", 0.8, K4, 256, 1.5, 4321, 3, False)                       # no marker: yesterday's key
    od._pair_pnp_fused(4, 5)
    t = od._step_begin(4, 5, params)
    od._step_end(params, t)
    assert [n for n, _ in od._ctx.log] == ["pnp_pair", "pnp_pair_begin", "pnp_pair_end"]
    assert od.pnp_lo_counts is None
    win = _odo(_rec(), pnp_refine=3, match_window=(24, 16), depth="sparse", loop_check=40)
    win._pair_pnp_fused(4, 5)
    win._step_end(win._pose_params(), win._step_begin(4, 5, win._pose_params()))
    assert [n for n, _ in win._ctx.log] == ["pnp_pair_window", "pnp_pair_begin_window", "pnp_pair_end"]


def test_rounds_reach_the_lo_entries_and_the_ticket_key():
    K4 = (500.0, 500.0, 320.0, 240.0)
    od = _odo(_rec(), pnp_refine=3, pnp_lo_rounds=2, cross_check=True)
    params = od._pose_params()
    assert params == ("pnp", 0.8, K4, 256, 1.5, 4321, 3, True, LoRounds(2))
    T = od._pair_pnp_fused(4, 5)
    want = dict(slot_a=4, slot_b=5, ratio=0.8, K4=K4, lo_rounds=2, iters=256, thr=1.5, seed=4321, refine=3, want_matches=False, cross_check=True,
                window=None, loop=None)
    assert od._ctx.log == [("pnp_pair_lo", want)]
    assert np.array_equal(T[:3], REF) and od.pnp_lo_counts == (3, 44) and od.skip_cause == "init"
    assert od._step_begin(4, 5, params) == 42 and od._ctx.log[-1] == ("pnp_pair_begin_lo", want)
    # the key of a step begun ahead differs with the rounds: 2 rounds never collect a ticket of 3, of none, or the reverse
    keys = {r: _odo(_rec(), pnp_refine=3, **({"pnp_lo_rounds": r} if r else {}))._pose_params() for r in (0, 1, 2, 3)}
    assert len(set(keys.values())) == 4
    od._specs[((4, 0), (5, 0), keys[3][:7] + (True,) + keys[3][8:])] = 6
    od._specs[((4, 0), (5, 0), params)] = 2
    od._pair_pnp_fused(4, 5)
    assert od._ctx.log[-1] == ("pnp_pair_end_lo", dict(ticket=2, want_matches=False)) and len(od._specs) == 1
    od._drop_specs()
    assert od._ctx.log[-1] == ("pnp_pair_end_lo", dict(ticket=6, want_matches=False)) and not od._specs
    # window and loop check travel as keywords of the same entries; the marker stays the last entry, LoopCheck before it
    win = _odo(_rec(), pnp_refine=3, pnp_lo_rounds=3, match_window=(24, 16), depth="sparse", loop_check=40)
    p = win._pose_params()
    assert p[-3:] == ((24.0, 16.0), LoopCheck(40), LoRounds(3))
    win._pair_pnp_fused(1, 2)
    name, kw = win._ctx.log[-1]
    assert name == "pnp_pair_lo" and (kw["window"], kw["loop"], kw["lo_rounds"]) == ((24.0, 16.0), 40, 3)


def test_decisions_are_unchanged_with_rounds():
    # "outlier" still reads the winner's count, whatever the rounds' support is
    od = _odo(_rec(best_count=9, support=60), pnp_refine=3, pnp_lo_rounds=3)
    assert od._pair_pnp_fused(0, 1) is None and od.skip_cause == "outlier"
    # the gates see the LO pose ...
    od = _odo(_rec(Rt_refined=_rt(0.02, 1.5)), pnp_refine=3, pnp_lo_rounds=3)
    assert od._pair_pnp_fused(0, 1) is None and od.skip_cause == "bigdist"
    # ... and the winner when no round completed
    for status in (1, -1):
        od = _odo(_rec(status=status, support=30, Rt_refined=_rt(0.02, 5.0)), pnp_refine=3, pnp_lo_rounds=3)
        T = od._pair_pnp_fused(0, 1)
        assert np.array_equal(T[:3], WIN) and od.pnp_lo_counts == (0, 30)


def test_the_fused_map_step_takes_the_lo_entry_only_with_rounds():
    rec = dict(_rec(), decision=0, view=np.array([100, 90], np.int32), update=np.array([40, 0, 1, 50, 0, 149], np.int32), update_flags=0,
               c_T_w=REF, w_T_c=REF)
    for rounds, entry in ((0, "map_track"), (3, "track_map_lo")):
        kw = dict(pnp_lo_rounds=rounds) if rounds else {}
        od = _odo(rec, pnp_refine=3, depth="sparse", track="map", map_fused=True, **kw)
        od._map, od._view_slot = 0, 3
        assert od._map_track_fused(5, (500.0, 500.0, 320.0, 240.0)) is True
        (name, a), = od._ctx.log
        assert name == entry and a.get("lo_rounds", 0) == rounds and a["refine"] == 3 and a["want_matches"] is False
        assert od.pnp_lo_counts == ((3, 44) if rounds else None)
