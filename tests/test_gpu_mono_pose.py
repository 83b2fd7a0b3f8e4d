"""Monocular pose recovery on the device: vo_recover_pose against LAPACK and against the numpy restatement, the fused pair step
against its composition, serials and ordering of steps in flight, and MonoOdometer's scale chain on C1 frames."""
import numpy as np
import pytest

import mono_pose_ref as ref
from openvo_amd import _native, calib, mono
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

K4 = [400.0, 400.0, 320.0, 240.0]
GATE = float(np.sin(np.deg2rad(0.5)) ** 2)
SIZES = (1, 5, 63, 64, 65, 1000, 8000)
MOTIONS = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1),
           "forward": (0.03, -0.02, -1)}


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 640, 480, 16, 2000)
    yield c
    c.close()


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _scene(n, motion, seed):
    """n correspondences in float32 pixels: 40 % true tracks of a rigid scene, 30 % planted behind a camera and masked out, 30 %
    wrong tracks masked in; keypoint indices (a permutation into na, nb > n keypoints) and depths of frame a for 70 % of them."""
    rng = np.random.default_rng(seed)
    R = calib.rodrigues_vec_to_mat(rng.normal(size=3) * rng.uniform(0.0, 0.2) / np.sqrt(3))
    t = np.asarray(MOTIONS[motion], np.float64)
    t = t / np.linalg.norm(t) * rng.uniform(0.2, 0.8)
    n_bad, n_wrong = int(0.3 * n), int(0.3 * n)
    Z = rng.uniform(4, 30, n)
    X = np.c_[rng.uniform(-0.55, 0.55, n) * Z, rng.uniform(-0.4, 0.4, n) * Z, Z]
    X[:n_bad] *= -1.0                                         # behind the first camera (they project, but they are no inliers)
    Y = X @ R.T + t
    p1 = X[:, :2] / X[:, 2:] * K4[0] + K4[2:]
    p2 = Y[:, :2] / Y[:, 2:] * K4[0] + K4[2:]
    p2[n_bad:n_bad + n_wrong] = rng.uniform([0, 0], [640, 480], (n_wrong, 2))
    mask = np.ones(n, np.uint8)
    mask[:n_bad] = 0
    order = rng.permutation(n)
    p1, p2, mask, Z = p1[order], p2[order], mask[order], np.abs(Z[order])
    na, nb = n + 7, n + 11
    q, ti = rng.permutation(na)[:n].astype(np.int32), rng.permutation(nb)[:n].astype(np.int32)
    depth_a = np.zeros(na)
    depth_a[q] = Z / np.linalg.norm(t) * 1.7 * rng.uniform(0.99, 1.01, n)   # the previous pair's baseline was 1 / 1.7 of this one's ...
    none = rng.random(na) < 0.3
    depth_a[none] = np.where(rng.random(int(none.sum())) < 0.5, 0.0, -1.0)   # ... and 30 % of the keypoints had no depth
    E = _skew(t / np.linalg.norm(t)) @ R
    return dict(E=E, p1=p1.astype(np.float32), p2=p2.astype(np.float32), mask=mask, q=q, t=ti, na=na, nb=nb, depth_a=depth_a, R=R,
                tdir=t / np.linalg.norm(t))


def _check_against_ref(got, s, depth_a, rel=1e-12):
    """the device's record and arrays against the numpy restatement fed the device's OWN pose"""
    r = ref.depths_and_scale(got["R"], got["t"], s["p1"], s["p2"], K4, s["mask"], s["q"], s["t"], s["na"], s["nb"], depth_a, GATE)
    assert got["n_depth"] == r["n_depth"] and got["n_shared"] == r["n_shared"]
    assert np.array_equal(got["depth_b"] != 0, r["depth_b"] != 0)                 # the valid set (t_idx names every keypoint once)
    for k in ("depth_b", "z1", "z2"):
        assert np.all(np.abs(got[k] - r[k]) <= rel * np.abs(r[k])), k
    assert abs(got["scale_rel"] - r["scale_rel"]) <= rel * abs(r["scale_rel"])
    return r


def test_recover_pose_on_synthetic_points(ctx):
    winners = set()
    for n in SIZES:
        for j, motion in enumerate(MOTIONS):
            s = _scene(n, motion, 100 * n + j)
            got = ctx.recover_pose(s["E"] * (-1.0 if j & 1 else 1.0), s["p1"], s["p2"], K4, s["mask"], s["q"], s["t"], s["na"], s["nb"],
                                   s["depth_a"], GATE)
            inl = s["mask"] != 0
            x1, x2 = ref.normalise(s["p1"], K4)[inl], ref.normalise(s["p2"], K4)[inl]
            # LAPACK on all inliers
            Rl, tl, good = mono.recover_pose(s["E"], x1, x2)
            assert got["flags"] == 0 and got["matches"] == n and got["best_count"] == int(inl.sum())
            assert np.abs(got["R"] - Rl).max() <= 1e-9 and np.abs(got["t"] - tl).max() <= 1e-9, (n, motion)
            assert np.abs(got["R"] - s["R"]).max() <= 1e-9 and np.abs(got["t"] - s["tdir"]).max() <= 1e-9, (n, motion)
            # votes and winner: exact, against the restatement's own decomposition (no vote of these scenes sits on the boundary)
            R1, R2, t = ref.decompose(s["E"] * (-1.0 if j & 1 else 1.0))
            for Rk in (R1, R2):
                z1, z2, _ = ref.depths(Rk, t, x1, x2)
                assert min(np.abs(z1).min(), np.abs(z2).min()) >= 1e-6
            votes4, winner = ref.vote(R1, R2, t, x1, x2, np.ones(len(x1), bool))
            assert np.array_equal(got["votes4"], votes4) and got["winner"] == winner and votes4[winner] == good, (n, motion)
            winners.add(got["winner"])
            r = _check_against_ref(got, s, s["depth_a"])
            if n >= 1000:                                       # (the true tracks outnumber the wrong ones that triangulate: the median is theirs)
                assert r["n_shared"] > 0.05 * n and abs(got["scale_rel"] / 1.7 - 1.0) < 0.02
    assert winners == {0, 1, 2, 3}, winners


def test_recover_pose_duplicates_missing_depths_and_median_parity(ctx):
    s = _scene(1000, "+x", 77)
    # several correspondences name one keypoint of b: the lowest i wins
    dup = s["t"].copy()
    good = np.nonzero(s["mask"])[0]
    dup[good[5:9]] = dup[good[3]]
    dup[good[50]] = dup[good[40]]
    got = ctx.recover_pose(s["E"], s["p1"], s["p2"], K4, s["mask"], s["q"], dup, s["na"], s["nb"], s["depth_a"], GATE)
    r = ref.depths_and_scale(got["R"], got["t"], s["p1"], s["p2"], K4, s["mask"], s["q"], dup, s["na"], s["nb"], s["depth_a"], GATE)
    assert got["n_depth"] == r["n_depth"] and np.array_equal(got["depth_b"] != 0, r["depth_b"] != 0)
    assert np.all(np.abs(got["depth_b"] - r["depth_b"]) <= 1e-12 * np.abs(r["depth_b"]))
    first = min(i for i in [good[3]] + list(good[5:9]) if r["valid"][i])
    assert got["depth_b"][dup[first]] == got["z2"][first] != 0
    # no mask, no indices: the identity
    ident = ctx.recover_pose(s["E"], s["p1"], s["p2"], K4)
    assert ident["flags"] == 4 and ident["best_count"] == 1000 and ident["n_shared"] == 0 and ident["scale_rel"] == 0.0
    ri = ref.depths_and_scale(ident["R"], ident["t"], s["p1"], s["p2"], K4, gate=0.0)
    assert ident["n_depth"] == ri["n_depth"] and np.all(np.abs(ident["depth_b"] - ri["depth_b"]) <= 1e-12 * np.abs(ri["depth_b"]))
    # n_shared even, odd and 0 (depth_a with zeros and negatives throughout)
    base = ref.depths_and_scale(got["R"], got["t"], s["p1"], s["p2"], K4, s["mask"], s["q"], s["t"], s["na"], s["nb"], s["depth_a"], GATE)
    shared = np.nonzero(base["valid"] & (s["depth_a"][s["q"]] > 0))[0]
    seen = set()
    for drop in (0, 1, len(shared)):
        d = s["depth_a"].copy()
        d[s["q"][shared[:drop]]] = -2.0
        g = ctx.recover_pose(s["E"], s["p1"], s["p2"], K4, s["mask"], s["q"], s["t"], s["na"], s["nb"], d, GATE)
        r = _check_against_ref(g, s, d)
        assert g["n_shared"] == len(shared) - drop and g["flags"] == 0
        seen.add("none" if g["n_shared"] == 0 else ("even", "odd")[g["n_shared"] & 1])
        if g["n_shared"] == 0:
            assert g["scale_rel"] == 0.0
    assert seen == {"even", "odd", "none"}
    # flags: no inlier; an index outside its frame (refused)
    g = ctx.recover_pose(s["E"], s["p1"], s["p2"], K4, np.zeros(1000, np.uint8), s["q"], s["t"], s["na"], s["nb"], s["depth_a"], GATE)
    assert g["flags"] & 1 and np.array_equal(g["R"], np.eye(3)) and not g["t"].any() and not g["depth_b"].any() and not g["z1"].any()
    bad = s["t"].copy()
    bad[17] = s["nb"]
    with pytest.raises(_native.VoError) as e:
        ctx.recover_pose(s["E"], s["p1"], s["p2"], K4, s["mask"], s["q"], bad, s["na"], s["nb"], s["depth_a"], GATE)
    assert e.value.code == -3


# ---- C1 frames ----------------------------------------------------------------------------------------------------------------
C1_FRAMES = (0, 1, 3, 4, 6, 7, 8)


@pytest.fixture(scope="module")
def c1():
    c = Corridor("C1")
    return c, [c.pair(k)[0] for k in C1_FRAMES]


def _c1_K4(c):
    return [c.f, c.f, c.cx, c.cy]


def _load(ctx, frames, first_slot=20):
    for s, f in enumerate(frames):
        ctx.upload_mono(first_slot + s, f)
        assert ctx.orb_slot_count(first_slot + s, 2000, 0) > 500


_REC_INTS = ("matches", "best_iter", "best_count", "winner", "n_depth", "n_shared", "flags")
_REC_ARRAYS = ("votes4", "E", "R", "t")


def _same_record(a, b):
    assert all(a[k] == b[k] for k in _REC_INTS), ([a[k] for k in _REC_INTS], [b[k] for k in _REC_INTS])
    assert all(np.array_equal(a[k], b[k]) for k in _REC_ARRAYS) and a["scale_rel"] == b["scale_rel"]


def test_fused_step_equals_its_composition(ctx, c1):
    c, frames = c1
    k4 = _c1_K4(c)
    _load(ctx, frames[:3])
    xy = [ctx.download_keypoints_xy(20 + s) for s in range(3)]
    for solver in (5, 8):
        for cross in (False, True):
            depth, serial, sync = None, 0, []
            for a in (0, 1):
                got = ctx.mono_pose_pair(20 + a, 21 + a, 0.8, k4, 1500, 1.0, 4321, solver, cross, prev_serial=serial, min_parallax_sin2=GATE)
                sync.append(got)
                comp = ctx.mono_pair(20 + a, 21 + a, 0.8, k4, 1500, 1.0, 4321, want_matches=True, solver=solver, cross_check=cross)
                rp = ctx.recover_pose(comp["E"], xy[a][comp["q"]], xy[a + 1][comp["t"]], k4, comp["mask"], comp["q"], comp["t"], len(xy[a]),
                                      len(xy[a + 1]), depth, GATE)
                assert (got["matches"], got["best_iter"], got["best_count"]) == (comp["matches"], comp["best_iter"], comp["best_count"])
                assert np.array_equal(got["E"], comp["E"]) and got["best_count"] > 100
                for k in ("winner", "n_depth", "n_shared", "flags"):
                    assert got[k] == rp[k], (k, solver, cross, a)
                for k in ("votes4", "R", "t"):
                    assert np.array_equal(got[k], rp[k]), (k, solver, cross, a)
                assert got["scale_rel"] == rp["scale_rel"]
                depth, serial_dev = ctx.download_mono_depth(21 + a)
                assert serial_dev == got["serial"] != 0 and np.array_equal(depth, rp["depth_b"])
                assert 0 < np.count_nonzero(depth) <= got["n_depth"]       # (fewer: without cross-check several matches may name one keypoint)
                if cross:
                    assert np.count_nonzero(depth) == got["n_depth"]
                serial = got["serial"]
            assert sync[0]["flags"] == 4 and sync[1]["flags"] == 0 and sync[1]["n_shared"] >= 20 and sync[1]["scale_rel"] > 0
            # the same in two halves, tickets ended out of order
            t0, s0 = ctx.mono_pose_pair_begin(20, 21, 0.8, k4, 1500, 1.0, 4321, solver, cross, prev_serial=0, min_parallax_sin2=GATE)
            t1, s1 = ctx.mono_pose_pair_begin(21, 22, 0.8, k4, 1500, 1.0, 4321, solver, cross, prev_serial=s0, min_parallax_sin2=GATE)
            assert 0 != s0 != s1 != 0
            with pytest.raises(_native.VoError):
                ctx.mono_pair_end(t1)                                   # a pose ticket is ended by mono_pose_pair_end
            g1, g0 = ctx.mono_pose_pair_end(t1), ctx.mono_pose_pair_end(t0)
            _same_record(g0, sync[0])
            _same_record(g1, sync[1])
            assert (g0["serial"], g1["serial"]) == (s0, s1)
            d2, ser2 = ctx.download_mono_depth(22)
            assert ser2 == s1 and np.array_equal(d2, depth)


def test_serials_and_ordering_of_three_steps_in_flight(ctx, c1):
    c, frames = c1
    k4 = _c1_K4(c)
    _load(ctx, frames[:4])
    args = (0.8, k4, 1500, 1.0, 4321, 5, False)
    one, serial = [], 0
    for a in range(3):
        one.append(ctx.mono_pose_pair(20 + a, 21 + a, *args, prev_serial=serial, min_parallax_sin2=GATE))
        serial = one[-1]["serial"]
    depth_one = ctx.download_mono_depth(23)[0]
    tickets, serial = [], 0
    for a in range(3):
        t, serial = ctx.mono_pose_pair_begin(20 + a, 21 + a, *args, prev_serial=serial, min_parallax_sin2=GATE)
        tickets.append(t)
    got = {a: ctx.mono_pose_pair_end(tickets[a]) for a in (2, 0, 1)}
    for a in range(3):
        _same_record(got[a], one[a])
    assert got[1]["flags"] == 0 and got[2]["flags"] == 0 and got[1]["n_shared"] >= 20 and got[2]["n_shared"] >= 20
    depth, ser = ctx.download_mono_depth(23)
    assert ser == got[2]["serial"] and np.array_equal(depth, depth_one)
    # a serial that is not the one slot 22's depths carry: no scale, everything else as before
    for wrong in (got[0]["serial"], got[2]["serial"] + 1000, 0):
        g = ctx.mono_pose_pair(22, 23, *args, prev_serial=wrong, min_parallax_sin2=GATE)
        assert g["flags"] == 4 and g["scale_rel"] == 0.0 and g["n_shared"] == 0
        assert np.array_equal(g["R"], one[2]["R"]) and g["n_depth"] == one[2]["n_depth"]
    ok = ctx.mono_pose_pair(22, 23, *args, prev_serial=got[1]["serial"], min_parallax_sin2=GATE)
    _same_record(ok, one[2])
    # ... and once the slot has been refilled (the same image: same keypoints) its old serial is refused as well
    ctx.upload_mono(22, frames[2])
    assert ctx.orb_slot_count(22, 2000, 0) > 500
    assert ctx.download_mono_depth(22)[1] == 0
    g = ctx.mono_pose_pair(22, 23, *args, prev_serial=got[1]["serial"], min_parallax_sin2=GATE)
    assert g["flags"] == 4 and g["scale_rel"] == 0.0 and g["n_shared"] == 0 and np.array_equal(g["R"], one[2]["R"])
    with pytest.raises(_native.VoError):
        ctx.mono_pose_pair(22, 22, *args, prev_serial=0, min_parallax_sin2=GATE)


def _cpu_chain(oracle, c, frames, min_inliers=30):
    """the odometer's chain from the CPU stages: ORB -> kNN-2 -> ratio -> essential RANSAC -> mono_pose_ref"""
    k4 = _c1_K4(c)
    kp = [oracle.orb_detect_and_compute(f, None, 2000) for f in frames]
    T, scale, depth, prev, log = np.eye(4), 1.0, None, 0, []
    for k in range(1, len(frames)):
        ri, rd = oracle.bf_knn2_hamming(kp[prev]["desc"], kp[k]["desc"])
        rq, rt = oracle.ratio_filter(ri, rd, 0.8)
        rr = oracle.ransac_essential(kp[prev]["xy"][rq], kp[k]["xy"][rt], k4, 1500, 1.0, 4321, solver=5)
        ok = len(rq) >= 6 and rr["best_count"] >= min_inliers
        r = ref.recover_pose(rr["E"], kp[prev]["xy"][rq], kp[k]["xy"][rt], k4, rr["mask"], rq, rt, len(kp[prev]["xy"]), len(kp[k]["xy"]),
                             depth, GATE)
        if ok:
            if not (r["flags"] & 4) and r["n_shared"] >= 20:
                scale *= r["scale_rel"]
            Tk = np.eye(4)
            Tk[:3, :3], Tk[:3, 3] = r["R"], r["t"] * scale
            T = Tk @ T
            depth, prev = r["depth_b"], k
        log.append((ok, r["n_shared"], r["scale_rel"], T.copy()))
    return log


def _gpu_chain(ctx, c, frames, spec, **kw):
    odo = mono.MonoOdometer(c.K(), (c.w, c.h), nfeatures=2000, ransac_iters=1500, context=ctx, **kw)
    odo.speculate = spec
    odo.stage_frames(frames)
    log = []
    for k in range(len(frames)):
        ok = odo.update(k)
        last = odo.last or {}
        log.append((ok, last.get("n_shared"), last.get("scale_rel"), odo.c_T_w.copy(), odo.scale, odo.scale_status, last.get("best_iter")))
    stats = dict(odo.speculation)
    odo.close()
    return log, stats


def _same_chain(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[:3] == y[:3] and np.array_equal(x[3], y[3]) and x[4:] == y[4:]


def test_odometer_scale_chain_on_c1(ctx, c1, oracle):
    c, frames = c1
    kw = dict(pose_on_device=True, propagate_scale=True)
    log0, _ = _gpu_chain(ctx, c, frames, 0, **kw)
    log3, stats = _gpu_chain(ctx, c, frames, 3, **kw)
    _same_chain(log0, log3)
    assert stats["used"] >= 3
    assert all(x[0] for x in log3)
    # against the reference composition on the CPU
    cpu = _cpu_chain(oracle, c, frames)
    for k, (g, r) in enumerate(zip(log3[1:], cpu)):
        print("pair %d: n_shared %d / %d, scale_rel %.6f / %.6f" % (k, g[1], r[1], g[2], r[2]))
    for g, r in zip(log3[1:], cpu):
        assert g[0] == r[0] and g[1] == r[1]
        assert abs(g[2] - r[2]) <= 1e-9 and np.abs(g[3] - r[3]).max() <= 1e-9
    # against the truth: the baselines of the frames chosen
    pos = [Corridor.gt_pose(k)[:3, 3] for k in C1_FRAMES]
    base = [np.linalg.norm(pos[k + 1] - pos[k]) for k in range(len(pos) - 1)]
    assert log3[1][5] == "held" and log3[1][4] == 1.0
    for k in range(1, len(base)):
        true = base[k] / base[k - 1]
        g = log3[k + 1]
        print("pair %d: log(scale_rel / true ratio %.4f) = %+.4f, %d shared tracks" % (k, true, np.log(g[2] / true), g[1]))
    for k in range(1, len(base)):
        g = log3[k + 1]
        assert g[5] == "tracked" and abs(np.log(g[2] / (base[k] / base[k - 1]))) < 0.1, k
    assert abs(np.log(log3[-1][4] / (base[-1] / base[0]))) < 0.3           # the chained scale: |t| of the last pair in units of the first
    # a rejected frame (blank: no keypoints) holds the reference and its depths
    blank = list(frames)
    blank.insert(3, np.zeros_like(frames[0]))
    b0, _ = _gpu_chain(ctx, c, blank, 0, **kw)
    b3, _ = _gpu_chain(ctx, c, blank, 3, **kw)
    _same_chain(b0, b3)
    assert [x[0] for x in b3] == [True, True, True, False, True, True, True, True]
    for with_blank, without in zip(b3[4:], log3[3:]):
        assert with_blank[1:3] == without[1:3] and np.array_equal(with_blank[3], without[3])


def test_odometer_with_the_keywords_off_is_todays(ctx, c1):
    c, frames = c1
    k4 = _c1_K4(c)
    a, _ = _gpu_chain(ctx, c, frames, 3)
    b, _ = _gpu_chain(ctx, c, frames, 3, pose_on_device=False, propagate_scale=False)
    _same_chain(a, b)
    # today's arithmetic written out: vo_mono_pair, the first 512 inliers, LAPACK on the host, |t| = 1
    _load(ctx, frames)
    T, prev = np.eye(4), 0
    xy = [ctx.download_keypoints_xy(20 + s).astype(np.float64) for s in range(len(frames))]
    for k in range(1, len(frames)):
        r = ctx.mono_pair(20 + prev, 20 + k, 0.8, k4, 1500, 1.0, 4321, want_matches=True, solver=5)
        assert r["best_iter"] == a[k][6] and r["best_count"] >= 30
        inl = np.nonzero(r["mask"])[0][:512]
        xa, xb = xy[prev][r["q"][inl]], xy[k][r["t"][inl]]
        R, t, _ = mono.recover_pose(r["E"].copy(), (xa - k4[2:]) / k4[:2], (xb - k4[2:]) / k4[:2])
        Tk = np.eye(4)
        Tk[:3, :3], Tk[:3, 3] = R, t / max(np.linalg.norm(t), 1e-300) * 1.0
        T = Tk @ T
        assert np.array_equal(T, a[k][3]), k
        prev = k
    assert a[-1][4] == 1.0 and a[-1][5] == "held" and a[-1][1] is None
