"""The numpy restatement of vo_recover_pose (tests/mono_pose_ref.py) held to known answers, and MonoOdometer's scale chain on a
scripted context.  No GPU."""
import numpy as np

import mono_pose_ref as ref
from openvo_amd import calib


def _rot(v):
    return calib.rodrigues_vec_to_mat(np.asarray(v, np.float64))


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _three_views(rng, forward, n=120):
    """exact normalised points of three views: depth 4-40 in view 0, baselines 0.1-1.0, rotations up to 0.2 rad"""
    Z = rng.uniform(4, 40, n)
    X = np.c_[rng.uniform(-0.5, 0.5, (n, 2)) * Z[:, None], Z]         # (a field of view that keeps every point in front of all three)
    views, motions = [X], []
    for _ in range(2):
        R = _rot(rng.normal(size=3) * rng.uniform(0.0, 0.2) / np.sqrt(3))
        if forward:
            t = np.array([rng.normal() * 0.02, rng.normal() * 0.02, -1.0])
        else:
            t = rng.normal(size=3)
        t *= rng.uniform(0.1, 1.0) / np.linalg.norm(t)
        views.append(views[-1] @ R.T + t)
        motions.append((R, t))
    return views, motions


_SCENES = None


def _scenes():
    global _SCENES
    if _SCENES is None:
        rng = np.random.default_rng(2024)
        _SCENES = [_three_views(rng, k % 3 == 2) for k in range(200)]
    return _SCENES


def _run_scene(views, motions, gate=0.0):
    out, depth = [], None
    for k, (R, t) in enumerate(motions):
        b = np.linalg.norm(t)
        E = _skew(t / b) @ R
        xa, xb = views[k][:, :2] / views[k][:, 2:], views[k + 1][:, :2] / views[k + 1][:, 2:]
        r = ref.recover_pose(E * (-1.0 if k else 1.0), xa, xb, None, depth_a=depth, gate=gate)    # (the sign of E is arbitrary)
        depth = r["depth_b"]
        out.append(r)
    return out


def test_pose_and_scale_of_exact_three_view_scenes():
    worst_rt = worst_s = 0.0
    for views, motions in _scenes():
        r1, r2 = _run_scene(views, motions)
        for r, (R, t) in zip((r1, r2), motions):
            assert r["flags"] & 3 == 0
            worst_rt = max(worst_rt, np.abs(r["R"] - R).max(), np.abs(r["t"] - t / np.linalg.norm(t)).max())
            assert r["votes4"][r["winner"]] == len(views[0]) and r["n_depth"] == len(views[0])
        assert r1["flags"] == 4 and r1["n_shared"] == 0 and r1["scale_rel"] == 0.0
        true = np.linalg.norm(motions[1][1]) / np.linalg.norm(motions[0][1])
        assert r2["flags"] == 0 and r2["n_shared"] == len(views[0])
        worst_s = max(worst_s, abs(r2["scale_rel"] / true - 1.0))
    print("worst |R, t - truth| %.3g, worst relative scale error %.3g" % (worst_rt, worst_s))
    assert worst_rt <= 1e-9 and worst_s <= 1e-9


def test_depths_times_baseline_are_the_true_depths():
    worst = 0.0
    for views, motions in _scenes():
        r1, _ = _run_scene(views, motions)
        b = np.linalg.norm(motions[0][1])
        x1, x2 = views[0][:, :2] / views[0][:, 2:], views[1][:, :2] / views[1][:, 2:]
        sin2 = ref.depths(r1["R"], r1["t"], x1, x2)[2]
        ok = sin2 >= 1e-6
        assert ok.sum() > 0
        worst = max(worst, np.abs(r1["z1"] * b / views[0][:, 2] - 1.0)[ok].max(), np.abs(r1["depth_b"] * b / views[1][:, 2] - 1.0)[ok].max())
    print("worst relative depth error %.3g" % worst)
    assert worst <= 1e-9


def _simple_pair(n=40, seed=5):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-3, 3, (n, 2)), rng.uniform(5, 20, n)]
    R, t = _rot([0.02, -0.05, 0.01]), np.array([0.6, 0.1, -0.2])
    Y = X @ R.T + t
    return X, Y, R, t, _skew(t / np.linalg.norm(t)) @ R


def test_duplicate_train_index_lowest_correspondence_wins():
    X, Y, R, t, E = _simple_pair()
    n = len(X)
    q, ti = np.arange(n), np.arange(n)
    ti[[7, 30, 31]] = 3                                      # correspondences 3, 7, 30 and 31 all name keypoint 3 of frame b
    ti[12] = 11
    r = ref.recover_pose(E, X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:], None, q_idx=q, t_idx=ti, na=n, nb=n)
    assert r["valid"].all()
    assert r["depth_b"][3] == r["z2"][3] and r["depth_b"][11] == r["z2"][11] != r["z2"][12]
    assert r["depth_b"][7] == 0 and r["depth_b"][30] == 0 and r["depth_b"][31] == 0 and r["depth_b"][12] == 0
    mask = np.ones(n, np.uint8)
    mask[3] = 0                                              # ... without 3, the next lowest: 7
    r = ref.recover_pose(E, X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:], None, mask=mask, q_idx=q, t_idx=ti, na=n, nb=n)
    assert r["depth_b"][3] == r["z2"][7] and r["n_depth"] == n - 1


def test_lower_median_even_odd_and_none():
    assert ref.lower_median([]) == 0.0
    assert ref.lower_median([3.0]) == 3.0
    assert ref.lower_median([4.0, 1.0]) == 1.0
    assert ref.lower_median([5.0, 1.0, 3.0]) == 3.0
    assert ref.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0
    X, Y, R, t, E = _simple_pair()
    x1, x2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    for m in (0, 1, 4, 5):
        d = np.zeros(len(X))
        d[:m] = X[:m, 2] * np.array([1.0, 7.0, 3.0, 5.0, 2.0])[:m]   # depth ratios 1, 7, 3, 5, 2 times the baseline
        d[m:m + 3] = [-1.0, 0.0, np.inf]                     # none
        r = ref.recover_pose(E, x1, x2, None, depth_a=d)
        assert r["n_shared"] == m
        want = {0: 0.0, 1: 1.0, 4: 3.0, 5: 3.0}[m] * np.linalg.norm(t)
        assert abs(r["scale_rel"] - want) <= 1e-12 * max(want, 1.0)


def test_parallax_gate_and_validity_on_hand_built_points():
    # camera moves 1 to the right (t = (-1, 0, 0)), no rotation: a point at depth Z straight ahead is seen under an angle
    # atan(1 / Z) from the two centres; a point on the baseline's axis would have none
    R, t = np.eye(3), np.array([-1.0, 0.0, 0.0])
    Z = np.array([2.0, 10.0, 100.0, 1000.0])
    X = np.c_[np.zeros(4), np.zeros(4), Z]
    Y = X + t
    x1, x2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    z1, z2, sin2 = ref.depths(R, t, x1, x2)
    assert np.allclose(z1, Z, rtol=1e-12) and np.allclose(z2, Z, rtol=1e-12)
    assert np.allclose(sin2, 1.0 / (1.0 + Z * Z), rtol=1e-12)            # sin^2 of the angle at the point
    gate = np.sin(np.deg2rad(0.5)) ** 2                                  # 0.5 degrees: Z = 100 passes (0.57 deg), Z = 1000 does not
    r = ref.depths_and_scale(R, t, x1, x2, None, mask=np.array([1, 0, 1, 1]), gate=gate)
    assert r["valid"].tolist() == [True, False, True, False] and r["n_depth"] == 2
    assert r["depth_b"].tolist() == [z2[0], 0.0, z2[2], 0.0] and r["z1"][1] == 0.0
    # behind a camera: never valid, whatever the gate
    r = ref.depths_and_scale(R, -t, x1, x2, None, gate=0.0)
    assert not r["valid"].any() and (r["z1"] < 0).all()


def test_flags_for_an_empty_mask_and_a_bad_index():
    X, Y, R, t, E = _simple_pair()
    n = len(X)
    x1, x2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    r = ref.recover_pose(E, x1, x2, None, mask=np.zeros(n, np.uint8), depth_a=np.ones(n))
    assert r["flags"] == 1 and np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and not r["depth_b"].any() and r["scale_rel"] == 0
    for bad_q, bad_t in ((n, 0), (-1, 0), (0, n), (0, -1)):
        q, ti = np.arange(n), np.arange(n)
        q[5] += bad_q and (bad_q - q[5])
        ti[9] += bad_t and (bad_t - ti[9])
        r = ref.recover_pose(E, x1, x2, None, q_idx=q, t_idx=ti, na=n, nb=n, depth_a=np.ones(n))
        assert r["flags"] == 2 and not r["depth_b"].any() and not r["z1"].any()
    r = ref.recover_pose(E, x1, x2, None)
    assert r["flags"] == 4 and r["n_depth"] == n


class _ScriptedPoseContext:
    """Stands in for the native context under MonoOdometer(pose_on_device=True): frames are their indices, a step's outcome is a
    function of the two frames it was begun on and of the serial it was handed -- flag bit 2 unless that serial is the one the
    latest step into slot a stamped (what the device checks)."""
    kp_cap = 64

    def __init__(self, rejected=(), shared=None, rel=None, no_scale=()):
        self.rejected, self.shared, self.rel, self.no_scale = set(rejected), shared or {}, rel or {}, set(no_scale)
        self.frame_of, self.open, self.begun, self.slot_serial = {}, {}, [], {}
        self.next_ticket, self.next_serial = 0, 0

    def stage_pairs(self, pairs):
        pass

    def lookahead_drop(self, slot):
        pass

    def _fill(self, slot, idx):
        self.frame_of[slot] = idx
        self.slot_serial.pop(slot, None)                      # a refill clears the slot's serial

    def load_staged_pair(self, slot, idx, pre):
        self._fill(slot, idx)

    def prefetch_staged_mono(self, slot, idx, nf):
        self._fill(slot, idx)

    def slot_ready(self, slot):
        return True

    def orb_slot_count(self, slot, nf, mode):
        return 40

    def download_keypoints_xy(self, slot):
        raise AssertionError("the device-pose mode keeps no keypoint positions on the host")

    def mono_pair_begin(self, *a, **k):
        raise AssertionError("the device-pose mode uses mono_pose_pair_begin")

    def mono_pose_pair_begin(self, a, b, ratio, K4, iters, thr, seed, solver=8, cross_check=False, prev_serial=0, min_parallax_sin2=0.0):
        assert len(self.open) < 5 and a != b
        assert abs(min_parallax_sin2 - np.sin(np.deg2rad(0.5)) ** 2) < 1e-15
        self.next_ticket += 1
        self.next_serial += 1
        fa, fb = self.frame_of[a], self.frame_of[b]
        ok = prev_serial != 0 and self.slot_serial.get(a) == prev_serial and fb not in self.no_scale
        self.open[self.next_ticket] = (fa, fb, self.next_serial, ok)
        self.begun.append((fa, fb, prev_serial, self.next_serial))
        self.slot_serial[b] = self.next_serial
        return self.next_ticket, self.next_serial

    def mono_pose_pair_end(self, ticket):
        fa, fb, serial, ok = self.open.pop(ticket)
        return dict(matches=30, best_iter=fa * 100 + fb, best_count=2 if fb in self.rejected else 25, winner=0, n_depth=25,
                    n_shared=self.shared.get(fb, 50) if ok else 0, flags=0 if ok else 4, serial=serial, votes4=np.array([25, 0, 0, 0]),
                    E=np.eye(3), R=np.eye(3), t=np.array([0.0, 0.0, 1.0]), scale_rel=self.rel.get(fb, 1.0) if ok else 0.0)

    def close(self):
        pass


def _drive(spec):
    from openvo_amd import mono
    ctx = _ScriptedPoseContext(rejected={6}, shared={3: 5}, rel={2: 2.0, 3: 9.0, 4: 9.0, 7: 0.5, 8: 4.0}, no_scale={4})
    odo = mono.MonoOdometer(np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]]), (64, 48), nfeatures=40, min_inliers=10, context=ctx,
                            pose_on_device=True, propagate_scale=True)
    assert odo._pool is None
    odo.speculate, odo.lookahead = spec, 5
    odo.stage_frames(list(range(12)))
    log = []
    for k in range(9):
        ok = odo.update(k, scale=3.0) if k == 5 else odo.update(k)
        log.append((ok, odo.scale, odo.scale_status))
    odo.restart()
    for k in (9, 10, 11):
        ok = odo.update(k)
        log.append((ok, odo.scale, odo.scale_status))
    pose = odo.c_T_w.copy()
    odo.close()
    assert not ctx.open, "steps left open"
    return log, pose, ctx.begun, dict(odo.speculation)


def test_mono_odometer_scale_chain_on_a_scripted_context():
    """tracked / held (too few tracks; flag bit 2) / anchored / a rejected frame / restart(), and the serial each step is given."""
    log0, pose0, begun0, _ = _drive(0)
    log3, pose3, begun3, spec3 = _drive(3)
    assert log0 == log3 and np.array_equal(pose0, pose3)
    assert spec3["used"] >= 4 and spec3["void"] >= 1 and len(begun3) > len(begun0)
    want = [(True, 1.0, "held"),         # frame 0: the first frame
            (True, 1.0, "held"),         # (0, 1): no predecessor
            (True, 2.0, "tracked"),      # (1, 2): ratio 2
            (True, 2.0, "held"),         # (2, 3): 5 shared tracks < 20
            (True, 2.0, "held"),         # (3, 4): flag bit 2
            (True, 3.0, "anchored"),     # (4, 5): update(scale=3)
            (False, 3.0, "anchored"),    # (5, 6): rejected, 5 stays the reference
            (True, 1.5, "tracked"),      # (5, 7): ratio 0.5 against the last accepted pair
            (True, 6.0, "tracked"),      # (7, 8): ratio 4
            (True, 6.0, "tracked"),      # frame 9 after restart(): a first frame
            (True, 6.0, "held"),         # (9, 10): no predecessor
            (True, 6.0, "tracked")]      # (10, 11): ratio 1
    assert log3 == want
    # translation chained: 1 + 2 + 2 + 2 + 3 + 1.5 + 6 + 6 + 6 along z
    assert abs(pose3[2, 3] - 29.5) < 1e-12
    # without speculation every step is handed the serial of the step that made its first frame the reference
    by_pair = {(fa, fb): (prev, ser) for fa, fb, prev, ser in begun0}
    assert by_pair[(0, 1)][0] == 0 and by_pair[(9, 10)][0] == 0
    assert by_pair[(1, 2)][0] == by_pair[(0, 1)][1] and by_pair[(5, 6)][0] == by_pair[(4, 5)][1]
    assert by_pair[(5, 7)][0] == by_pair[(4, 5)][1] and by_pair[(10, 11)][0] == by_pair[(9, 10)][1]
    # with speculation each step begun ahead got the serial of the step it assumed accepted: the latest one begun into its slot a
    # ((5, 7) is begun again after frame 6 was rejected, (9, 10) after restart(): checked on their own)
    latest = {}
    for fa, fb, prev, ser in begun3:
        assert prev == latest.get(fa, 0) or (fa, fb) in ((5, 7), (9, 10)), (fa, fb)
        latest[fb] = ser
    last = {x[:2]: x for x in begun3}
    assert last[(5, 7)][2] == last[(4, 5)][3] and last[(9, 10)][2] == 0 and last[(10, 11)][2] == last[(9, 10)][3]


def test_propagate_scale_needs_the_device_pose():
    import pytest
    from openvo_amd import mono
    with pytest.raises(ValueError):
        mono.MonoOdometer(np.eye(3), (64, 48), context=_ScriptedPoseContext(), propagate_scale=True)
