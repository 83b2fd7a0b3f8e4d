"""The loop check (VO_MATCH_LOOP: a temporal match is kept only when the right partners of its two keypoints look alike) on the GPU:
the three pair steps on two sparse C1 slots against the composed path -- the matches of the plain path gated in numpy on the
downloaded kp_rdesc (tests/sparse_loop_ref.py::loop_gate) --, the statuses of the flag, tickets that keep their threshold, and
StereoOdometer(loop_check=) against the CPU chain.  All on ctx_small."""
import numpy as np
import pytest

import pnp_refine_ref as PR
import pose_fit_ref as PF
import sparse_loop_ref as X
import sparse_stereo_ref as S
from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.features import BFMatcher
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

VO_E_ARG, VO_E_STATE = -1, -3
PARAMS = (4, 100, 2.0, 75)
RATIO, ITERS, THR, SEED = 0.8, 256, 1.5, 4321
WINDOW = (24, 16)
A, B, DENSE = 10, 11, 12


def _camera(ctx, name):
    c = Corridor(name)
    return c, StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def two(ctx_small):
    """C1 frames 0 and 1 as sparse slots 10 and 11 (host copies of what they hold), frame 1 once more as the dense slot 12"""
    ctx = ctx_small
    c, cam = _camera(ctx, "C1")
    ctx.set_sparse_assoc(False, None)
    pairs = c.pairs(0, 2)
    fr = []
    for s, (L, R) in zip((A, B), pairs):
        ctx.upload_pair(s, L, R, True)
        ctx.sparse_stereo(s, 500, *PARAMS)
        f = ctx.download_keypoints(s)
        f["xyz"], f["disp"] = ctx.download_keypoint_depth(s)
        f["rdesc"] = ctx.download_keypoint_rdesc(s)
        fr.append(f)
    ctx.upload_pair(DENSE, *pairs[1], True)
    ctx.sgbm_compute(DENSE)
    ctx.orb_slot_count(DENSE, 500, 0)
    Q = cam.Q
    yield dict(c=c, cam=cam, fr=fr, K4=[Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]], roi=S.crop_bounds(cam.valid_region_left, c.w, c.h))
    if ctx._loop is not None:
        ctx.clear_match_loop()


def _plain_matches(ctx, fa, fb, cross, window):
    """the matches of the step without the loop check, composed from the matcher's own seams"""
    if window is None:
        idx, dist = ctx.bf_knn2(fa["desc"], fb["desc"])
        mutual = ctx.bf_knn2_mutual(fa["desc"], fb["desc"])[2] if cross else None
    elif cross:
        idx, dist, mutual, _ = ctx.bf_knn2_window(fa["desc"], fb["desc"], fa["xy"], fb["xy"], window, True)
    else:
        (idx, dist), mutual = ctx.bf_knn2_window(fa["desc"], fb["desc"], fa["xy"], fb["xy"], window), None
    ok = (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float32).astype(np.float64) < RATIO * dist[:, 1].astype(np.float32).astype(np.float64))
    if mutual is not None:
        ok &= mutual > 0
    q = np.nonzero(ok)[0].astype(np.int32)
    return q, idx[q, 0]


CASES = [(False, None), (True, None), (False, WINDOW), (True, WINDOW)]


@pytest.mark.parametrize("cross,window", CASES)
def test_point_clouds_with_the_loop_check(ctx_small, two, cross, window):
    ctx, (fa, fb) = ctx_small, two["fr"]
    q0, t0 = _plain_matches(ctx, fa, fb, cross, window)
    plain = ctx.point_clouds(A, B, RATIO, cross, window)
    assert np.array_equal(plain[0], q0) and np.array_equal(plain[1], t0) and len(q0) >= 40
    sizes = []
    for thr in (0, 48, 256):
        wq, wt = X.loop_gate(fa, fb, q0, t0, thr)
        q, t, pa, pb, sa, sb = ctx.point_clouds(A, B, RATIO, cross, window, loop=thr)
        assert np.array_equal(q, wq) and np.array_equal(t, wt)
        assert np.array_equal(_bits(pa), _bits(fa["xyz"][q])) and np.array_equal(_bits(pb), _bits(fb["xyz"][t]))
        assert not sa.any() and not sb.any()
        sizes.append(len(q))
    print("cross %s window %s: M %d; loop <= 0 / 48 / 256: %s" % (cross, window, len(q0), sizes))
    assert sizes[0] <= sizes[1] <= sizes[2] == len(q0) and sizes[1] >= 20
    if not cross and window is None:
        assert sizes[0] < sizes[1] < sizes[2]                   # the check has work to do at 48, and 0 asks for identical partners
    for got, want in zip(ctx.point_clouds(A, B, RATIO, cross, window, loop=256), plain):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("cross,window", CASES)
@pytest.mark.parametrize("thr2", [(0.0, 0.0), (0.1, 0.02)])
def test_pose_pair_with_the_loop_check(ctx_small, two, thr2, cross, window):
    """counts, status and the transform (np.array_equal) against the composed path on the gated matches: vo_rigid_clique, then the
    fits in the fused step's own summation order (tests/pose_fit_ref.py); _begin / _end the same; 256 is the plain call"""
    ctx, (fa, fb) = ctx_small, two["fr"]
    q0, t0 = _plain_matches(ctx, fa, fb, cross, window)
    for thr in (0, 48, 256):
        q, t = X.loop_gate(fa, fb, q0, t0, thr)
        counts, rc, T1, T2 = ctx.pose_pair(A, B, RATIO, 10, *thr2, cross, window, loop=thr)
        c2, rc2, T1b, T2b = ctx.pose_pair_end(ctx.pose_pair_begin(A, B, RATIO, 10, *thr2, cross, window, loop=thr))
        assert np.array_equal(c2, counts) and np.array_equal(rc2, rc)
        assert rc[1] != 0 or np.array_equal(T2b, T2)                # (no fit, no transform: the record's T2 is then undefined)
        assert counts[0] == len(q) and counts[3] == 0
        if len(q) < 10:
            continue
        pa, pb = fa["xyz"][q], fb["xyz"][t]
        if thr2[0] > 0:
            keep = ctx.rigid_clique(pa, pb, thr2[0]) > 0
            pa, pb = pa[keep], pb[keep]
        assert counts[1] == len(pa)
        if len(pa) >= 10:
            r_n2, r_rc1, r_rc2, r_T = PF.pose_fit(pa, pb, thr2[1])
            assert (r_n2, r_rc1, r_rc2) == (int(counts[2]), int(rc[0]), int(rc[1]))
            if r_n2 >= 10:
                assert np.array_equal(T2, r_T)
        if thr == 256:
            p_counts, p_rc, _, p_T2 = ctx.pose_pair(A, B, RATIO, 10, *thr2, cross, window)
            assert np.array_equal(counts, p_counts) and np.array_equal(rc, p_rc) and rc[1] == 0 and np.array_equal(T2, p_T2)
        elif thr == 48:
            assert 20 <= counts[0] <= len(q0) and rc[1] == 0


@pytest.mark.parametrize("cross,window", CASES)
def test_pnp_pair_with_the_loop_check(ctx_small, two, cross, window):
    ctx, (fa, fb) = ctx_small, two["fr"]
    q0, t0 = _plain_matches(ctx, fa, fb, cross, window)
    kw = dict(iters=ITERS, thr=THR, seed=SEED, refine=3, want_matches=True, cross_check=cross)
    for thr in (0, 48, 256):
        q, t = X.loop_gate(fa, fb, q0, t0, thr)
        r = ctx.pnp_pair_window(A, B, RATIO, two["K4"], window, loop=thr, **kw)
        r2 = ctx.pnp_pair_end(ctx.pnp_pair_begin_window(A, B, RATIO, two["K4"], window, loop=thr, **kw), want_matches=True)
        for k in ("matches", "n", "best_iter", "best_count", "flags", "refine_status", "refine_steps"):
            assert r[k] == r2[k], k
        for k in ("Rt", "Rt_refined", "mask", "q", "t"):
            assert np.array_equal(r[k], r2[k], equal_nan=(k != "q" and k != "t" and k != "mask")), k
        Xa = fa["xyz"][q]
        ok = np.isfinite(Xa).all(axis=1)
        assert (r["matches"], r["n"], r["flags"]) == (len(q), int(ok.sum()), 0)
        assert np.array_equal(r["q"], q[ok]) and np.array_equal(r["t"], t[ok])
        if r["n"] >= 4:
            uv = (fb["xy"][t[ok]] + np.array(two["roi"][:2], np.float32)).astype(np.float32)
            want = ctx.ransac_pnp(Xa[ok], uv, two["K4"], ITERS, THR, SEED)
            assert (r["best_iter"], r["best_count"]) == (want["best_iter"], want["best_count"])
            assert np.array_equal(r["mask"], want["mask"]) and np.array_equal(r["Rt"], want["Rt"])
            if r["refine_status"] == 0:
                ref, status, steps = PR.refine(r["Rt"], Xa[ok], uv, two["K4"], r["mask"], 3)
                assert (status, steps) == (0, r["refine_steps"]) and np.abs(r["Rt_refined"] - ref).max() <= 1e-9
        if thr == 256:
            plain = ctx.pnp_pair_window(A, B, RATIO, two["K4"], window, **kw)
            for k in r:
                assert np.array_equal(r[k], plain[k], equal_nan=isinstance(r[k], np.ndarray) and r[k].dtype.kind == "f"), k
        elif thr == 48:
            assert 20 <= r["matches"] <= len(q0) and r["best_count"] >= 10


def test_statuses_of_the_flag(ctx_small, two):
    ctx, K4 = ctx_small, two["K4"]
    lib, h = ctx._lib, ctx._h
    for bad in (-1, 257):
        assert lib.vo_set_match_loop(h, bad) == VO_E_ARG
    assert lib.vo_set_match_loop(None, 48) == VO_E_ARG and lib.vo_clear_match_loop(None) == VO_E_ARG
    n = _native.ctypes.c_int(0)
    for slot in (-1, 28, 2 ** 31 - 1, -2 ** 31):
        assert lib.vo_download_keypoint_rdesc(h, slot, None, 0, _native.ctypes.byref(n)) == VO_E_ARG
    assert lib.vo_download_keypoint_rdesc(None, A, None, 0, None) == VO_E_ARG
    assert lib.vo_download_keypoint_rdesc(h, A, None, -1, None) == 0                    # (the count only: nothing is written)
    assert lib.vo_download_keypoint_rdesc(h, A, _native._p(np.zeros((4, 32), np.uint8)), 4, _native.ctypes.byref(n)) == -4 and n.value > 4
    if ctx._loop is not None:
        ctx.clear_match_loop()
    assert lib.vo_clear_match_loop(h) == VO_E_STATE
    # the flag without a threshold: VO_E_ARG from every entry that takes it
    m, c4, rc2, T = _native.ctypes.c_int(0), np.zeros(4, np.int32), np.zeros(2, np.int32), np.zeros(12)
    tk, K = _native.ctypes.c_int(-1), np.ascontiguousarray(K4, np.float64)
    p = _native._p
    assert lib.vo_point_clouds_ex(h, A, B, RATIO, 4, None, None, None, None, None, None, 0, _native.ctypes.byref(m)) == VO_E_ARG
    assert lib.vo_pose_pair_ex(h, A, B, RATIO, 4, 10, 0.0, 0.0, p(c4), p(rc2), None, p(T)) == VO_E_ARG
    assert lib.vo_pose_pair_begin_ex(h, A, B, RATIO, 4, 10, 0.0, 0.0, _native.ctypes.byref(tk)) == VO_E_ARG
    assert lib.vo_pnp_pair_begin(h, A, B, RATIO, 4, p(K), ITERS, THR, SEED, 0, 0, _native.ctypes.byref(tk)) == VO_E_ARG
    assert lib.vo_pose_pair_ex(h, A, B, RATIO, 8, 10, 0.0, 0.0, p(c4), p(rc2), None, p(T)) == VO_E_ARG          # an unknown bit
    # with a threshold: VO_E_STATE on dense slots (both, or one of the two), VO_E_ARG in the monocular entries and the kNN seams
    for a, b in ((DENSE, DENSE), (A, DENSE), (DENSE, B)):
        for call in (lambda: ctx.point_clouds(a, b, RATIO, loop=48), lambda: ctx.pose_pair(a, b, RATIO, 10, 0, 0, loop=48),
                     lambda: ctx.pose_pair_begin(a, b, RATIO, 10, 0, 0, loop=48), lambda: ctx.pnp_pair_window(a, b, RATIO, K4, None, loop=48),
                     lambda: ctx.pnp_pair_begin_window(a, b, RATIO, K4, None, loop=48)):
            with pytest.raises(_native.VoError) as e:
                call()
            assert e.value.code == VO_E_STATE
    assert ctx._loop == 48
    out = np.zeros(64, np.float64)
    assert lib.vo_mono_pose_pair(h, A, B, RATIO, 4, p(K), 100, 1.0, SEED, 8, 0, 0.0, p(out)) == VO_E_ARG
    us = _native.ctypes.c_double(0)
    assert lib.vo_measure_knn_ex(h, A, B, 1, 4, _native.ctypes.byref(us)) == VO_E_ARG
    # nothing above left a ticket open or the slots unusable
    assert len(ctx.point_clouds(A, B, RATIO, loop=48)[0]) >= 20
    ctx.clear_match_loop()
    assert len(ctx.point_clouds(A, B, RATIO)[0]) >= 40


def test_a_ticket_keeps_the_threshold_it_was_begun_with(ctx_small, two):
    ctx, K4 = ctx_small, two["K4"]
    want_pose = ctx.pose_pair(A, B, RATIO, 10, 0.1, 0.02, loop=48)
    want_pnp = ctx.pnp_pair_window(A, B, RATIO, K4, None, ITERS, THR, SEED, loop=48)
    t1 = ctx.pose_pair_begin(A, B, RATIO, 10, 0.1, 0.02, loop=48)
    t2 = ctx.pnp_pair_begin_window(A, B, RATIO, K4, None, ITERS, THR, SEED, loop=48)
    ctx.set_match_loop(0)
    t3 = ctx.pose_pair_begin(A, B, RATIO, 10, 0.1, 0.02, loop=0)
    ctx.clear_match_loop()
    for got, want in zip(ctx.pose_pair_end(t1), want_pose):
        assert np.array_equal(got, want)
    got = ctx.pnp_pair_end(t2)
    for k in ("matches", "n", "best_iter", "best_count"):
        assert got[k] == want_pnp[k]
    assert np.array_equal(got["Rt"], want_pnp["Rt"])
    assert ctx.pose_pair_end(t3)[0][0] < want_pose[0][0]


# ---- the odometer ------------------------------------------------------------------------------------------------------------------
MODES = {"default": {}, "clique": dict(rigidity_threshold=0.1, outlier_threshold=0.02), "pnp": dict(pose_method="pnp"),
         "pnp-cross-window": dict(pose_method="pnp", cross_check=True, match_window=WINDOW)}


@pytest.fixture(scope="module")
def c1(ctx_small):
    ctx = ctx_small
    c, cam = _camera(ctx, "C1")
    frames = c.pairs(0, 8)
    x0, y0, x1, y1 = S.crop_bounds(cam.valid_region_left, c.w, c.h)
    cache = {}
    for L, R in frames:
        Lc, Rc = np.ascontiguousarray(L[y0:y1, x0:x1]), np.ascontiguousarray(R[y0:y1, x0:x1])
        f = X.sparse_stereo_ex(Lc, Rc, ctx.orb_host(Lc, None, 500), ctx.orb_host(Rc, None, 500), cam.Q, x0, y0, *PARAMS, 3, 0.8)
        f["origin"] = (x0, y0)
        cache[id(L)] = f
    yield dict(cam=cam, frames=frames, cache=cache)
    ctx.set_sparse_assoc(False, None)
    if ctx._loop is not None:
        ctx.clear_match_loop()


def _state(odo, ok):
    return ok, odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()


@pytest.mark.parametrize("name", list(MODES))
def test_odometer_with_everything_on_against_the_cpu_chain(ctx_small, oracle, c1, name):
    """StereoOdometer(depth="sparse", sparse_mutual=True, sparse_ratio=0.8, loop_check=48) over C1 frames 0-7: flags, skip_cause
    and c_T_w (1e-9) against the CPU chain; run(depth=4) equals the update() chain exactly"""
    cam, frames, kw = c1["cam"], c1["frames"], MODES[name]
    ref = X.SparseLoopOdometer(oracle, cam.Q, cam.valid_region_left, frames=c1["cache"], mutual=True, ratio=0.8, loop_check=48, **kw)
    on = dict(preprocessed_frames=True, depth="sparse", sparse_mutual=True, sparse_ratio=0.8, loop_check=48, **kw)
    odo = StereoOdometer(cam, **on)
    got = []
    for k, (L, R) in enumerate(frames):
        g, w = _state(odo, odo.update(L, R)), _state(ref, ref.update(L, R))
        assert g[:3] == w[:3], (name, k, g[:3], w[:3])
        assert np.abs(g[3] - w[3]).max() <= 1e-9, (name, k)
        got.append(g)
    assert sum(g[0] for g in got) >= 7
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(frames) - 1)
    print("%s: end-point error %.3f m" % (name, np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3])))
    odo.reset_lookahead()
    ran = StereoOdometer(cam, **on)
    for k, ok in enumerate(ran.run(iter(frames), depth=4)):
        r = _state(ran, ok)
        assert r[:3] == got[k][:3] and np.array_equal(r[3], got[k][3]), (name, k)
    assert ctx_small.lookahead_depth() == 0


class _OtherMatcher(BFMatcher):
    """a replaced matcher: the odometer takes the generic path"""


@pytest.mark.parametrize("name", ["default", "pnp"])
def test_a_replaced_matcher_equals_the_fused_path(ctx_small, c1, name):
    cam, frames, kw = c1["cam"], c1["frames"][:5], MODES[name]
    on = dict(preprocessed_frames=True, depth="sparse", sparse_mutual=True, sparse_ratio=0.8, loop_check=48, **kw)
    fused = StereoOdometer(cam, **on)
    want = [_state(fused, fused.update(L, R)) for L, R in frames]
    generic = StereoOdometer(cam, **on)
    generic.matcher = _OtherMatcher(ctx_small)
    for k, (L, R) in enumerate(frames):
        g = _state(generic, generic.update(L, R))
        assert g[:3] == want[k][:3] and np.abs(g[3] - want[k][3]).max() <= 1e-9, (name, k)
    assert sum(w[0] for w in want) >= 4
