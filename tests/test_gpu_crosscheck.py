"""Cross-check matching (mutual nearest neighbours) on the GPU, against the CPU oracle.

The kernel computes a(j), the nearest query of every train descriptor, from the same distance tiles as the kNN-2 (column
minima), so the independent check is the oracle's kNN with the roles swapped: oracle.bf_knn2_hamming(t, q)[:, 0] is a(j) with
the lower-index tie rule.  The odometer chains are checked against oracle/odometer.py's RefStereoOdometer with its
point_clouds filtered by that back-match (the reference itself cannot cross-check: cv2 refuses knnMatch(k=2) with it)."""
import numpy as np
import pytest

from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu


def _mutual_ref(oracle, q, t):
    """-> (idx, dist, mutual, t_best) from the oracle alone"""
    idx, dist = oracle.bf_knn2_hamming(q, t)
    if len(t) and len(q):
        bi, bd = oracle.bf_knn2_hamming(t, q)
        t_best = np.stack([bi[:, 0], bd[:, 0]], 1).astype(np.int32)
    else:
        t_best = np.tile(np.array([-1, 0x7FFFFFFF], np.int32), (len(t), 1))
    b = idx[:, 0]
    mutual = np.array([b[i] >= 0 and t_best[b[i], 0] == i for i in range(len(q))], np.uint8)
    return idx, dist, mutual, t_best


def _check(ctx, oracle, q, t, what):
    gi, gd, gm, gt = ctx.bf_knn2_mutual(q, t)
    ri, rd, rm, rt = _mutual_ref(oracle, q, t)
    pi, pd = ctx.bf_knn2(q, t)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd), what
    assert np.array_equal(gi, pi) and np.array_equal(gd, pd), what             # the kNN-2 of the same launch = the plain kernel's
    assert np.array_equal(gt, rt), (what, int((gt != rt).any(1).sum()))
    assert np.array_equal(gm, rm), (what, int((gm != rm).sum()))
    return gm


def test_mutual_kernel_tile_and_slice_edges_and_adversarial_bit_patterns(oracle):
    """Every train's a(j) and distance, every query's flag, and the kNN-2 of the same call, bit for bit, over the tile / slice /
    group edges of the plain kernel's edge test (nt = 1, nq = 1, 9000-row train sets, 8012 x 8030), all-zero / all-one /
    single-bit descriptors, duplicated train rows, duplicated QUERIES (a(j) ties -> the lower query index) and a set against
    itself."""
    ctx = _native.Context(0, 640, 480, 64, 9000)
    rng = np.random.default_rng(78)
    sizes = [(64, 16), (65, 17), (63, 15), (512, 512), (513, 511), (130, 33), (3, 1), (5, 2), (700, 17), (1, 4097), (2, 8200),
             (1100, 2050), (8012, 8030), (576, 9000), (1, 1), (9000, 40)]
    for nq, nt in sizes:
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        q[0] = 0; t[0] = 255
        if nq > 2:
            q[1] = 255; q[2] = 0; q[2, 17] = 0x10
        if nt > 9:
            t[7] = t[2]; t[9] = 0
            t[nt - 1] = t[nt - 2]
        if nq > 70:
            q[69] = q[3]; q[nq - 1] = q[5]                       # duplicated queries, one of them across the last group's end
            q[66] = t[min(4, nt - 1)]                            # an exact match (distance 0) ...
            q[68] = t[min(4, nt - 1)]                            # ... twice: a(4) must be query 66
        _check(ctx, oracle, q, t, (nq, nt))
    d = rng.integers(0, 256, (700, 32), dtype=np.uint8)          # a set against itself: every query is its own mutual match
    assert _check(ctx, oracle, d, d, "self").all()
    z = np.zeros((300, 32), np.uint8); z[100:] = 255             # only two distinct rows on each side: ties everywhere
    _check(ctx, oracle, z, z[::-1].copy(), "ties")
    _check(ctx, oracle, d[:5], np.empty((0, 32), np.uint8), "empty train")
    ctx.close()


def test_mutual_words_under_uneven_load(oracle):
    """60 launches of changing size while the look-ahead engines run disparity + ORB beside them, every word checked: the
    per-launch reset of the column words (on the launching stream) and the atomics hold across launches and streams."""
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=4000)
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True)
    staged = cam.stage_pairs(c.pairs(0, 24))
    ctx = cam._ctx
    rng = np.random.default_rng(6)
    base = rng.integers(0, 256, (4000, 32), dtype=np.uint8)
    k = 0
    for rep in range(60):
        if rep % 3 == 0:
            odo.update(staged[k % 24], None)
            k += 1
        nq, nt = int(rng.integers(65, 2000)), int(rng.integers(40, 4000))
        q = base[rng.integers(0, 4000, nq)] ^ (rng.integers(0, 256, (nq, 32), dtype=np.uint8) & rng.integers(0, 256, (nq, 32), dtype=np.uint8) & 0x11)
        t = base[rng.permutation(4000)[:nt]]
        _check(ctx, oracle, q, t, (rep, nq, nt))
    assert ctx.sgbm_sweep_status() == 0
    ctx.close()


def _xref_class():
    from oracle import oracle as O
    from oracle.odometer import RefStereoOdometer

    class XRefStereoOdometer(RefStereoOdometer):
        """RefStereoOdometer whose point_clouds keeps only the ratio-test survivors whose m[0] is a mutual nearest neighbour"""
        pairs_seen = 0
        pairs_thinned = 0

        def point_clouds(self, f1, f2):
            idx, dist = O.bf_knn2_hamming(f1["desc"], f2["desc"])
            q, t = O.ratio_filter(idx, dist, self.match_threshold)
            back = O.bf_knn2_hamming(f2["desc"], f1["desc"])[0][:, 0]
            keep = back[t] == q
            self.pairs_seen += 1
            self.pairs_thinned += int(not keep.all())
            q, t = q[keep], t[keep]
            if len(q) < self.min_matches:
                return None, None
            p1, s1 = f1["d3"].sample(f1["kps"]["xy"][q])
            p2, s2 = f2["d3"].sample(f2["kps"]["xy"][t])
            if (s1 == 2).any() or (s2 == 2).any():
                raise ZeroDivisionError("division by zero")
            self.last_matches = (q, t)
            return p1, p2
    return XRefStereoOdometer


class _CachedRefCamera:
    """RefStereoCamera whose (slow) per-frame result is shared by several oracle odometers."""

    def __init__(self, rcam):
        self.rcam, self.cache, self.disp16 = rcam, {}, {}
        self.Q, self.valid_region_left = rcam.Q, rcam.valid_region_left

    def compute_3d(self, L, R, preprocessed=False):
        key = (L.ctypes.data, R.ctypes.data)
        if key not in self.cache:
            self.cache[key] = self.rcam.compute_3d(L, R, preprocessed=preprocessed)
            self.disp16[key] = self.rcam.last_disp16
        self.last_disp16 = self.disp16[key]
        return self.cache[key]


@pytest.mark.parametrize("name,first,n", [("C1", 0, 8), ("C2", 20, 5)])
def test_stereo_chain_with_cross_check_through_update_and_run(name, first, n):
    """C1 and C2 chains with cross_check=True, through update() (the fused synchronous step) and through run() (pose steps begun
    ahead, keyed by their parameters): accept / skip decisions, skip_cause, M and the chained pose (1e-9) equal the subclassed
    oracle's.  The default chain on the same camera afterwards is still the plain oracle's."""
    from oracle.odometer import RefStereoCamera, RefStereoOdometer
    XRef = _xref_class()
    c = Corridor(name)
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
    rcam = _CachedRefCamera(RefStereoCamera(cam.Q, cam.valid_region_left, c.sgbm_params()))
    frames = c.pairs(first, n)
    kw = dict(preprocessed_frames=True, rigidity_threshold=0.1, outlier_threshold=0.02)
    rodo = XRef(rcam, **kw)
    want = []
    for L, R in frames:
        want.append((rodo.update(L, R), rodo.skip_cause, rodo.c_T_w.copy()))
    assert rodo.pairs_thinned > 0                                 # the cross-check does remove matches on this sequence
    # update(): the fused synchronous step
    odo = StereoOdometer(cam, cross_check=True, **kw)
    rodo2 = XRef(rcam, **kw)
    for k, (L, R) in enumerate(frames):
        a, b = odo.update(L, R), rodo2.update(L, R)
        assert a == b == want[k][0] and odo.skip_cause == rodo2.skip_cause and odo.skipped_frames == rodo2.skipped_frames, (name, k)
        assert np.allclose(odo.c_T_w, want[k][2], rtol=0, atol=1e-9), (name, k)
    # M of every step equals the filtered oracle's match count (the last pair of each accepted update)
    odo_m = StereoOdometer(cam, cross_check=True, **kw)
    rodo3 = XRef(rcam, **kw)
    for k, (L, R) in enumerate(frames):
        odo_m.update(L, R); rodo3.update(L, R)
        if (k and rodo3.prev is not None and odo_m.prev_kps is not None and odo_m.prev_kps.frame.live
                and odo_m.current_kps.frame.live):
            counts = cam._ctx.pose_pair(odo_m.prev_kps.frame.slot, odo_m.current_kps.frame.slot, *odo_m._pose_params())[0]
            qf, tf = _filtered(rodo3.prev["desc"], rodo3.cur["desc"], 0.8)
            assert int(counts[0]) == len(qf), (name, k)
    # run(): steps begun ahead carry the flag in their key
    odo = StereoOdometer(cam, cross_check=True, **kw)
    got = [(ok, odo.skip_cause, odo.c_T_w.copy()) for ok in odo.run(iter(frames), depth=4)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and (g[0] or g[1] == w[1]), (name, k)
        assert np.allclose(g[2], w[2], rtol=0, atol=1e-9), (name, k)
    # the default is untouched: the plain oracle, and a run() right after the cross-checked one reuses no step of it
    plain = RefStereoOdometer(rcam, **kw)
    ref_plain = [(plain.update(L, R), plain.c_T_w.copy()) for L, R in frames]
    odo = StereoOdometer(cam, **kw)
    got = [(ok, odo.c_T_w.copy()) for ok in odo.run(iter(frames), depth=4)]
    for (ga, gT), (ra, rT) in zip(got, ref_plain):
        assert ga == ra and np.allclose(gT, rT, rtol=0, atol=1e-9)
    assert cam._ctx.sgbm_sweep_status() == 0


def _filtered(da, db, ratio):
    from oracle import oracle as O
    idx, dist = O.bf_knn2_hamming(da, db)
    q, t = O.ratio_filter(idx, dist, ratio)
    back = O.bf_knn2_hamming(db, da)[0][:, 0]
    keep = back[t] == q
    return q[keep], t[keep]


def test_point_clouds_seam_and_pnp_with_cross_check(oracle):
    """The point_clouds seam and pose_method="pnp" take the cross-checked match set: (q, t) of every step equal the oracle's
    filtered set, and the PnP chain still follows the corridor."""
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
    ctx = cam._ctx
    frames = c.pairs(0, 10)
    pnp = StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp", cross_check=True)
    checked = []
    real = ctx.point_clouds

    def spy(sa, sb, ratio, cross_check=False):
        out = real(sa, sb, ratio, cross_check)
        da, db = ctx.download_keypoints(sa)["desc"], ctx.download_keypoints(sb)["desc"]
        qf, tf = _filtered(da, db, ratio)
        assert cross_check and np.array_equal(out[0], qf) and np.array_equal(out[1], tf)
        idx, dist = oracle.bf_knn2_hamming(da, db)
        checked.append(len(oracle.ratio_filter(idx, dist, ratio)[0]) - len(qf))
        return out
    ctx.point_clouds = spy
    try:
        for L, R in frames:
            assert pnp.update(L, R), pnp.skip_cause
        x3, d, left = cam.compute_3d(*c.pair(11), preprocessed=True)
        odo = StereoOdometer(cam, preprocessed_frames=True, cross_check=True)
        kps, desc = odo.orb.detectAndCompute(left, odo.feature_mask(d))
        pa, pb = odo.point_clouds(pnp.current_kps, kps, pnp.current_desc, desc, pnp.current_3d, x3)
        assert pa is not None and len(pa) == len(pb) >= 10
    finally:
        del ctx.point_clouds
    assert len(checked) >= 10 and sum(checked) > 0                # every step went through the check; some matches were removed
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(9)
    assert np.linalg.norm(pnp.current_pose()[:3, 3] - gt[:3, 3]) < 0.05


@pytest.fixture(scope="module")
def c5():
    c = Corridor("C5")
    ctx = _native.Context(0, c.w, c.h, 16, 8000)
    frames = [c.pair(k)[0] for k in (0, 1)]
    yield c, ctx, frames
    ctx.close()


def test_mono_pair_with_cross_check_at_c5(oracle, c5):
    """mono_pair_ex with the cross-check at C5 (8000 keypoints, solvers 5 and 8) equals the oracle composition kNN -> ratio ->
    cross-check -> ransac_essential: M, winner, inlier count, mask, q / t, E to 1e-12; begin / end gives the synchronous result;
    and MonoOdometer(cross_check=True) uses it."""
    from openvo_amd.mono import MonoOdometer
    c, ctx, frames = c5
    for s, f in enumerate(frames):
        ctx.upload_mono(s, f)
        assert ctx.orb_slot_count(s, 8000, 0) > 7000
    K4 = [c.f, c.f, c.cx, c.cy]
    ref = [oracle.orb_detect_and_compute(f, None, 8000) for f in frames]
    rq, rt = _filtered(ref[0]["desc"], ref[1]["desc"], 0.8)
    plain_m = len(oracle.ratio_filter(*oracle.bf_knn2_hamming(ref[0]["desc"], ref[1]["desc"]), 0.8)[0])
    assert 1000 < len(rq) < plain_m
    for solver in (8, 5):
        got = ctx.mono_pair(0, 1, 0.8, K4, 5000, 1.0, 4321, want_matches=True, solver=solver, cross_check=True)
        rr = oracle.ransac_essential(ref[0]["xy"][rq], ref[1]["xy"][rt], K4, 5000, 1.0, 4321, solver=solver)
        assert got["matches"] == len(rq) and np.array_equal(got["q"], rq) and np.array_equal(got["t"], rt)
        assert got["best_iter"] == rr["best_iter"] and got["best_count"] == rr["best_count"], solver
        assert np.array_equal(got["mask"], rr["mask"]) and np.allclose(got["E"], rr["E"], rtol=0, atol=1e-12)
        tk = ctx.mono_pair_begin(0, 1, 0.8, K4, 5000, 1.0, 4321, want_matches=True, solver=solver, cross_check=True)
        ga = ctx.mono_pair_end(tk, want_matches=True)
        assert ga["matches"] == got["matches"] and ga["best_iter"] == got["best_iter"] and ga["best_count"] == got["best_count"]
        assert np.array_equal(ga["mask"], got["mask"]) and np.array_equal(ga["q"], got["q"]) and np.array_equal(ga["t"], got["t"])
        assert np.array_equal(ga["E"], got["E"])
        assert ctx.mono_pair(0, 1, 0.8, K4, 5000, 1.0, 4321, solver=solver)["matches"] == plain_m      # the default is untouched
    K = np.array([[c.f, 0, c.cx], [0, c.f, c.cy], [0, 0, 1.0]])
    odo = MonoOdometer(K, (c.w, c.h), nfeatures=8000, context=ctx, cross_check=True)
    for f in frames:
        assert odo.update(f), odo.skip_cause
    assert odo.last["matches"] == len(rq)


def test_cross_check_launch_cost(c5):
    """vo_measure_knn_ex: the cross-check form of the kernel at 8000 x 8000 costs clearly less than a second launch would."""
    c, ctx, frames = c5
    for s, f in enumerate(frames):
        ctx.upload_mono(s, f)
        assert ctx.orb_slot_count(s, 8000, 0) > 7000
    plain = min(ctx.measure_knn(0, 1, 50) for _ in range(3))
    cross = min(ctx.measure_knn(0, 1, 50, cross_check=True) for _ in range(3))
    print("knn 8000x8000: plain %.1f us, cross-check %.1f us (%.2fx)" % (plain, cross, cross / plain))
    assert cross < 2.0 * plain
