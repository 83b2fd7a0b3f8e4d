"""Sparse stereo depth on the GPU: vo_sparse_stereo against the numpy restatement (tests/sparse_stereo_ref.py) fed with the
library's own ORB of the two crops; the pair steps on slots whose keypoints carry depth against the composed path; and
StereoOdometer(depth="sparse") against the CPU chain.  T0 and C1 rigs on one context, Context(0, 640, 480, 64, 500)."""
import numpy as np
import pytest

import pnp_refine_ref as PR
import pose_fit_ref as PF
import sparse_stereo_ref as S
from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

VO_E_STATE = -3
PARAMS = (4, 100, 2.0, 75)
RATIO, ITERS, THR, SEED = 0.8, 256, 1.5, 4321
KP = ("xy", "size", "angle", "response", "octave", "desc")


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 640, 480, 64, 500)
    yield c
    c.close()


def _camera(ctx, name):
    c = Corridor(name)
    return c, StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sparse_slot_vs_restatement(ctx, slot, L, R, Q, roi, nfeatures):
    """upload + sparse_stereo into `slot`, the restatement on the downloaded crops with the library's ORB -> (got, want)"""
    h, w = L.shape
    ctx.upload_pair(slot, L, R, True)
    c3 = ctx.sparse_stereo(slot, nfeatures, *PARAMS)
    got = ctx.download_keypoints(slot)
    got["xyz"], got["disp"] = ctx.download_keypoint_depth(slot)
    Ld, Rd = ctx.download_left(slot, (h, w)), ctx.download_left(slot, (h, w), right=True)
    assert np.array_equal(Ld, L) and np.array_equal(Rd, R)
    want = S.sparse_frame(None, Ld, Rd, Q, roi, nfeatures, *PARAMS, orb=lambda img: ctx.orb_host(img, None, nfeatures))
    assert np.array_equal(c3, want["counts3"]), (c3, want["counts3"])
    for k in KP:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["disp"]), _bits(want["disp"]))
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"]))
    return got, want


def test_sparse_stereo_equals_the_restatement(ctx):
    """3 T0 frames and 4 C1 frames: kept set and order, all keypoint arrays and descriptors, kp_disp / kp_xyz as bit patterns,
    counts3.  One C1 frame with a ROI inset from the image; C1 at nfeatures = 500 has left keypoints of all 8 octaves."""
    c, cam = _camera(ctx, "T0")
    for k, (L, R) in enumerate(c.pairs(0, 3)):
        got, want = _sparse_slot_vs_restatement(ctx, k, L, R, cam.Q, cam.valid_region_left, 300)
        print("T0 frame %d: counts3 %s" % (k, want["counts3"]))
        assert want["counts3"][2] >= 40
    c, cam = _camera(ctx, "C1")
    octaves = set()
    for k, (L, R) in enumerate(c.pairs(0, 4)):
        roi = cam.valid_region_left
        if k == 2:
            roi = (40, 30, c.w - 50, c.h - 20)
            ctx.set_roi(*roi)
        got, want = _sparse_slot_vs_restatement(ctx, 4 + k, L, R, cam.Q, roi, 500)
        print("C1 frame %d: counts3 %s, octaves kept %s" % (k, want["counts3"], sorted(set(want["octave"].tolist()))))
        assert want["counts3"][2] >= 200
        x0, y0, x1, y1 = S.crop_bounds(roi, c.w, c.h)
        kl = ctx.orb_host(np.ascontiguousarray(L[y0:y1, x0:x1]), None, 500)
        octaves |= set(kl["octave"].tolist())
        if k == 2:
            ctx.set_roi(*cam.valid_region_left)
            assert (x0, y0) == (40, 30) and got["xyz"][:, 2].min() > 0
    assert octaves == set(range(8))


@pytest.fixture(scope="module")
def two(ctx):
    """C1 frames 0 and 1 as sparse slots 10 and 11 (host copies of what they hold), frame 1 once more as the dense slot 12"""
    c, cam = _camera(ctx, "C1")
    pairs = c.pairs(0, 2)
    fr = []
    for s, (L, R) in zip((10, 11), pairs):
        ctx.upload_pair(s, L, R, True)
        ctx.sparse_stereo(s, 500, *PARAMS)
        f = ctx.download_keypoints(s)
        f["xyz"], f["disp"] = ctx.download_keypoint_depth(s)
        fr.append(f)
    ctx.upload_pair(12, *pairs[1], True)
    ctx.sgbm_compute(12)
    ctx.orb_slot_count(12, 500, 0)
    Q = cam.Q
    return dict(c=c, cam=cam, fr=fr, K4=[Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]], roi=S.crop_bounds(cam.valid_region_left, c.w, c.h))


def _matches(ctx, fa, fb, cross=False):
    idx, dist = ctx.bf_knn2(fa["desc"], fb["desc"])
    q, t = ctx.ratio_filter(idx, dist, RATIO)
    if cross:
        mutual = ctx.bf_knn2_mutual(fa["desc"], fb["desc"])[2]
        keep = mutual[q] > 0
        q, t = q[keep], t[keep]
    return q, t


def test_point_clouds_on_sparse_slots(ctx, two):
    fa, fb = two["fr"]
    for cross in (False, True):
        q, t, pa, pb, sa, sb = ctx.point_clouds(10, 11, RATIO, cross)
        wq, wt = _matches(ctx, fa, fb, cross)
        assert len(q) >= 50 and np.array_equal(q, wq) and np.array_equal(t, wt)
        assert np.array_equal(_bits(pa), _bits(fa["xyz"][q])) and np.array_equal(_bits(pb), _bits(fb["xyz"][t]))
        assert not sa.any() and not sb.any()


def _composed_pose(ctx, pa, pb, rigidity, outlier, min_matches=10):
    """StereoOdometer.point_cloud_transform without the gates -> (n1, n2, T or None)"""
    if rigidity > 0:
        keep = ctx.rigid_clique(pa, pb, rigidity) > 0
        pa, pb = pa[keep], pb[keep]
    n1 = len(pa)
    if outlier > 0 and n1 >= 10:
        T = np.vstack([ctx.umeyama(pa, pb, True)[0], [0, 0, 0, 1]])
        hb = np.hstack([pb, np.ones((len(pb), 1))]).astype(np.float64)
        ha = np.hstack([pa, np.ones((len(pa), 1))]).astype(np.float64)
        err = np.linalg.norm(hb - ha @ T.T, axis=1) / np.linalg.norm(hb, axis=1)
        keep = err < outlier + np.median(err)
        pa, pb = pa[keep], pb[keep]
    if len(pa) < min_matches:
        return n1, len(pa), None
    return n1, len(pa), ctx.umeyama(pa, pb, True)[0]


@pytest.mark.parametrize("thr", [(0.0, 0.0), (0.1, 0.02)])
def test_pose_pair_on_sparse_slots(ctx, two, thr):
    """The composed path is kp_xyz indexed by the matches, then vo_rigid_clique, then the Umeyama fit(s).  Counts, flags and status
    are exact.  The transform is compared bit for bit (np.array_equal) with the composed path whose fits run in the fused step's
    own summation order (tests/pose_fit_ref.py: dev_umeyama_block / pose_fit_block restated in numpy on the clique's survivors);
    vo_umeyama sums in another order (device sums, host finish), so against IT the transform is within 1e-9, the bar of every
    fused pose in this project, and that difference is printed."""
    fa, fb = two["fr"]
    q, t = _matches(ctx, fa, fb)
    pa, pb = fa["xyz"][q], fb["xyz"][t]
    n1, n2, T = _composed_pose(ctx, pa, pb, *thr)
    counts, rc, _, T2 = ctx.pose_pair(10, 11, RATIO, 10, *thr)
    assert list(counts) == [len(q), n1, n2, 0] and rc[1] == 0 and T is not None
    if thr[0] > 0:
        keep = ctx.rigid_clique(pa, pb, thr[0]) > 0
        pa, pb = pa[keep], pb[keep]
    r_n2, r_rc1, r_rc2, r_T = PF.pose_fit(pa, pb, thr[1])
    print("pose_pair %s: M %d, n1 %d, n2 %d, |T - vo_umeyama path| = %.3e, |T - restated fused order| = %.3e" % (
        thr, len(q), n1, n2, np.abs(T2 - T).max(), np.abs(T2 - r_T).max()))
    assert (r_n2, r_rc1, r_rc2) == (n2, int(rc[0]), int(rc[1]))
    assert np.array_equal(T2, r_T)
    assert np.abs(T2 - T).max() <= 1e-9
    ticket = ctx.pose_pair_begin(10, 11, RATIO, 10, *thr)
    c2, rc2, _, T3 = ctx.pose_pair_end(ticket)
    assert np.array_equal(c2, counts) and np.array_equal(rc2, rc) and np.array_equal(T3, T2)


@pytest.mark.parametrize("refine", [0, 3])
def test_pnp_pair_on_sparse_slots(ctx, two, refine):
    fa, fb = two["fr"]
    q, t = _matches(ctx, fa, fb)
    X = fa["xyz"][q]
    ok = np.isfinite(X).all(axis=1)
    uv = (fb["xy"][t[ok]] + np.array(two["roi"][:2], np.float32)).astype(np.float32)
    want = ctx.ransac_pnp(X[ok], uv, two["K4"], ITERS, THR, SEED)
    r = ctx.pnp_pair(10, 11, RATIO, two["K4"], ITERS, THR, SEED, refine=refine, want_matches=True)
    assert (r["matches"], r["n"], r["flags"]) == (len(q), int(ok.sum()), 0) and r["n"] >= 50
    assert np.array_equal(r["q"], q[ok]) and np.array_equal(r["t"], t[ok])
    assert (r["best_iter"], r["best_count"]) == (want["best_iter"], want["best_count"])
    assert np.array_equal(r["mask"], want["mask"]) and np.array_equal(r["Rt"], want["Rt"])
    if refine:
        ref, status, steps = PR.refine(r["Rt"], X[ok], uv, two["K4"], r["mask"], refine)
        assert (r["refine_status"], r["refine_steps"]) == (status, steps) == (0, refine)
        assert np.abs(r["Rt_refined"] - ref).max() <= 1e-9
    else:
        assert (r["refine_status"], r["refine_steps"]) == (1, 0)
    r2 = ctx.pnp_pair_end(ctx.pnp_pair_begin(10, 11, RATIO, two["K4"], ITERS, THR, SEED, refine=refine, want_matches=True), want_matches=True)
    for k in ("matches", "n", "best_iter", "best_count", "flags", "refine_status", "refine_steps"):
        assert r[k] == r2[k], k
    for k in ("Rt", "Rt_refined", "mask", "q", "t"):
        assert np.array_equal(r[k], r2[k]), k


def test_mixed_slots_are_refused_and_orb_clears_the_mark(ctx, two):
    for a, b in ((10, 12), (12, 10)):
        for call in (lambda: ctx.point_clouds(a, b, RATIO), lambda: ctx.pose_pair(a, b, RATIO, 10, 0, 0), lambda: ctx.pose_pair_begin(a, b, RATIO, 10, 0, 0),
                     lambda: ctx.pnp_pair(a, b, RATIO, two["K4"]), lambda: ctx.pnp_pair_begin(a, b, RATIO, two["K4"])):
            with pytest.raises(_native.VoError) as e:
                call()
            assert e.value.code == VO_E_STATE
    # two dense slots: today's path (slot 13 = the same pair as slot 12)
    ctx.upload_pair(13, *two["c"].pair(1), True)
    ctx.sgbm_compute(13)
    ctx.orb_slot_count(13, 500, 0)
    q, t, pa, pb, sa, sb = ctx.point_clouds(12, 13, RATIO)
    assert len(q) >= 100 and np.array_equal(q, t)
    with pytest.raises(_native.VoError) as e:
        ctx.download_keypoint_depth(12)
    assert e.value.code == VO_E_STATE
    # ORB into a sparse slot: the keypoints are the left extraction again and carry no depth
    ctx.upload_pair(14, *two["c"].pair(0), True)
    c3 = ctx.sparse_stereo(14, 500, *PARAMS)
    assert len(ctx.download_keypoint_depth(14)[1]) == c3[2] < c3[0]
    assert ctx.orb_slot_count(14, 500, 0) == c3[0]
    with pytest.raises(_native.VoError) as e:
        ctx.download_keypoint_depth(14)
    assert e.value.code == VO_E_STATE
    # ... and a refill clears it too
    ctx.sparse_stereo(14, 500, *PARAMS)
    ctx.upload_pair(14, *two["c"].pair(1), True)
    with pytest.raises(_native.VoError) as e:
        ctx.download_keypoint_depth(14)
    assert e.value.code == VO_E_STATE


# ---- the odometer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(ctx, oracle):
    c, cam = _camera(ctx, "C1")
    return dict(c=c, cam=cam, frames=c.pairs(0, 8), cache={})


def _chain(odo, frames):
    return [(odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()) for L, R in frames]


@pytest.mark.parametrize("name,kw", [("pnp", dict(pose_method="pnp")), ("umeyama", {}),
                                     ("umeyama-clique", dict(rigidity_threshold=0.1, outlier_threshold=0.02)),
                                     ("pnp-cross", dict(pose_method="pnp", cross_check=True)),
                                     ("umeyama-window", dict(match_window=(24, 16)))])
def test_sparse_odometer_equals_the_cpu_chain(ctx, oracle, c1, name, kw):
    """C1 frames 0-7: accept flags, skip_cause and skipped_frames equal the CPU chain (restatement on the oracle's ORB + oracle
    matching and pose), c_T_w to 1e-9; run() equals update(); a dense odometer on the same camera before and after is unmoved."""
    cam, frames = c1["cam"], c1["frames"]
    dense_kw = dict(preprocessed_frames=True, rigidity_threshold=0.1, outlier_threshold=0.02)
    before = _chain(StereoOdometer(cam, **dense_kw), frames[:3])
    ref = S.SparseRefOdometer(oracle, cam.Q, cam.valid_region_left, frames=c1["cache"], **kw)
    want = _chain(ref, frames)
    odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **kw)
    got = _chain(odo, frames)
    assert sum(w[0] for w in want) >= 6, [w[:3] for w in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w[:3], (name, k, g[:3], w[:3])          # accept flag, skip_cause (on every frame), skipped_frames
        assert np.allclose(g[3], w[3], rtol=0, atol=1e-9), (name, k, np.abs(g[3] - w[3]).max())
    assert odo.current_3d.shape == (len(odo.current_kps), 3) and odo.current_disparity.shape == (len(odo.current_kps),)
    f = c1["cache"][id(frames[-1][0])]
    assert np.array_equal(np.asarray(odo.current_3d), f["xyz"]) and np.array_equal(np.asarray(odo.current_disparity), f["disp"])
    assert np.array_equal(odo.current_kps.xy, f["xy"]) and np.array_equal(np.asarray(odo.current_desc), f["desc"])
    odo2 = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **kw)
    ran = [(ok, odo2.skip_cause, odo2.skipped_frames, odo2.c_T_w.copy()) for ok in odo2.run(iter(frames), depth=4)]
    for g, r in zip(got, ran):
        assert g[:3] == r[:3] and np.array_equal(g[3], r[3])
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(frames) - 1)
    print("%s: end-point error %.3f m" % (name, np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3])))
    after = _chain(StereoOdometer(cam, **dense_kw), frames[:3])
    for b, a in zip(before, after):
        assert b[:3] == a[:3] and np.array_equal(b[3], a[3])
    assert ctx.sgbm_sweep_status() == 0


def test_compute_sparse_results_and_staged_pairs(ctx, oracle, c1):
    cam, frames = c1["cam"], c1["frames"]
    kps, desc, xyz, disp, left = cam.compute_sparse(*frames[0], 500, preprocessed=True)
    f = c1["cache"].get(id(frames[0][0])) or S.sparse_frame(oracle, *frames[0], cam.Q, cam.valid_region_left, 500, *PARAMS)
    assert len(kps) == len(desc) == xyz.shape[0] == disp.shape[0] >= 200 and xyz.shape == (len(kps), 3)
    assert np.array_equal(np.asarray(xyz), f["xyz"]) and np.array_equal(np.asarray(disp), f["disp"]) and np.array_equal(kps.xy, f["xy"])
    assert np.array_equal(np.asarray(desc), f["desc"])
    assert np.array_equal(np.asarray(left), cam.crop_to_valid_region_left(frames[0][0]))
    staged = cam.stage_pairs(frames[:2])
    k2, d2, x2, s2, _ = cam.compute_sparse(staged[0], None, 500, preprocessed=True)
    assert np.array_equal(np.asarray(x2), np.asarray(xyz)) and np.array_equal(np.asarray(d2), np.asarray(desc))
    assert cam.next_lookahead_slots() == []                   # nothing was started ahead
    sp = cam.submit(*frames[1], preprocessed=True)
    try:
        with pytest.raises(ValueError):
            cam.compute_sparse(sp, None, 500)
    finally:
        cam.release_submitted(sp)
    cam.reset_lookahead()
