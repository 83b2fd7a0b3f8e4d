"""Windowed matching on the GPU: k_bf_knn2<CROSS, WINDOW = true> against tests/window_match_ref.py bit for bit, and every
consumer of the window (stereo chains through update() and run(), the fallback's span, PnP, the monocular steps) against the
CPU oracle composed with that helper."""
import ctypes
import os
import sys

import numpy as np
import pytest

from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_match_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 1), (63, 15), (65, 17), (130, 33), (513, 511), (700, 17), (1, 4097), (1100, 2050), (2100, 4100)]
WINDOWS = [(0.0, 0.0), (24.0, 16.0), (64.0, 3.0), (3.0, 64.0), (1e6, 1e6)]
# the input conditions are asserted at the three sizes with the most (query, train) pairs: with a single query "one query with
# no candidate AND one with exactly one" cannot hold
BIG = sorted(SIZES, key=lambda s: s[0] * s[1])[-3:]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 640, 480, 64, 4200)
    yield c
    c.close()


def _inputs(nq, nt, seed):
    """descriptors and positions (uniform in 640 x 480) with duplicated descriptors, duplicated positions, a query on a train's
    position, NaN coordinates, a query with no train anywhere near and one with exactly one"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    xy_q = (rng.random((nq, 2)) * [640, 480]).astype(np.float32)
    xy_t = (rng.random((nt, 2)) * [640, 480]).astype(np.float32)
    q[0] = 0; t[0] = 255
    if nt > 9:
        t[7] = t[2]; t[nt - 1] = t[nt - 2]
    if nq > 5:
        q[4] = t[min(4, nt - 1)]
    if nq > 70:
        q[69] = q[3]; q[nq - 1] = q[5]
        q[66] = t[min(4, nt - 1)]; q[68] = t[min(4, nt - 1)]       # an exact match twice: a(4) must be the lower query
        xy_q[69] = xy_q[3]; xy_q[68] = xy_q[66]                    # ... from the same position
    if nt > 12:
        xy_t[11] = xy_t[10]; xy_t[7] = xy_t[2] + np.float32(1)     # duplicated positions; the duplicated descriptors side by side
        if nq > 13:
            xy_q[12] = xy_t[10]; xy_q[13] = xy_q[12]               # a radius-0 hit, twice
    if nt > 2:
        xy_t[2, 0] = np.nan
    elif nq > 1:
        xy_q[1, 1] = np.nan
    if nq > 20:
        xy_q[20, 1] = np.nan
    if nq > 31 and nt > 30:
        xy_q[30] = (-500, -500)                                    # nothing near
        xy_q[31] = (-1000, -1000); xy_t[30] = (-1000, -990)        # exactly one train near
    return q, t, xy_q, xy_t


def _edge(xy_q, xy_t, rx, ry):
    """query 0 and train 0 exactly (rx, ry) apart (in); train 1 one float32 step farther in x (out)"""
    xy_q, xy_t = xy_q.copy(), xy_t.copy()
    xy_q[0] = (100, 200)
    xy_t[0] = (np.float32(100) + np.float32(rx), np.float32(200) - np.float32(ry))
    if len(xy_t) > 1:
        xy_t[1] = (np.nextafter(np.float32(100) + np.float32(rx), np.float32(np.inf)), 200)
    m = W.window_mask(xy_q[:1], xy_t[:2], rx, ry)[0]
    assert m[0] and not m[1:].any()
    return xy_q, xy_t


def _compare(ctx, q, t, xy_q, xy_t, win, what, table):
    ri, rd, rm, rt = W.window_knn2_mutual(q, t, xy_q, xy_t, *win, table=table)
    gi, gd = ctx.bf_knn2_window(q, t, xy_q, xy_t, win)
    assert np.array_equal(gi, ri), (what, int((gi != ri).any(1).sum()))
    assert np.array_equal(gd, rd), (what, int((gd != rd).any(1).sum()))
    xi, xd, xm, xt = ctx.bf_knn2_window(q, t, xy_q, xy_t, win, cross_check=True)
    assert np.array_equal(xi, ri) and np.array_equal(xd, rd), what
    assert np.array_equal(xt, rt), (what, int((xt != rt).any(1).sum()))
    assert np.array_equal(xm, rm), (what, int((xm != rm).sum()))
    return ri, rd, rm, rt


@pytest.mark.parametrize("nq,nt", SIZES)
def test_windowed_kernel_equals_the_helper_bit_for_bit(ctx, nq, nt):
    """idx, dist, mutual and t_best of the windowed launch (plain and cross-check form) for five windows, with the rows as drawn
    (no tile can be skipped) and sorted by (y, x) (most tiles are): tile / group / slice / chunk edges, an exact-radius pair and
    its one-step-farther neighbour, NaN coordinates, duplicated descriptors and positions."""
    q, t, xy_q0, xy_t0 = _inputs(nq, nt, 1000 + nq + nt)
    D = W.hamming_table(q, t)
    pq = np.lexsort((xy_q0[:, 0], xy_q0[:, 1]))
    pt = np.lexsort((xy_t0[:, 0], xy_t0[:, 1]))
    for win in WINDOWS:
        xy_q, xy_t = _edge(xy_q0, xy_t0, *win)
        ri, rd, rm, rt = _compare(ctx, q, t, xy_q, xy_t, win, (nq, nt, win, "as drawn"), D)
        # (the positions the window moved belong to query 0 and trains 0, 1: the order stays sorted but for them)
        si, sd, sm, st = _compare(ctx, q[pq], t[pt], xy_q[pq], xy_t[pt], win, (nq, nt, win, "sorted"), D[np.ix_(pq, pt)])
        if win == (24.0, 16.0) and (nq, nt) in BIG:
            mask = W.window_mask(xy_q, xy_t, *win)
            cand = mask.sum(1)
            assert (cand == 0).any() and (cand == 1).any(), (nq, nt)
            pi, _ = W.window_knn2(q, t, xy_q, xy_t, 1e30, 1e30, table=D)
            finite = ~np.isnan(xy_q).any(1)
            assert (ri[finite, 0] != pi[finite, 0]).any(), (nq, nt)
            # sorted and as-drawn results agree after un-permuting: every distance, and every index whose distance is unique
            # among the query's candidates (a tie goes to the lower index, which is another train in another order)
            assert np.array_equal(sd, rd[pq]), (nq, nt)
            unique = np.zeros((nq, 2), bool)
            for k in range(2):
                unique[:, k] = (ri[:, k] >= 0) & ((mask & (D == rd[:, k][:, None])).sum(1) == 1)
            back = np.where(si >= 0, pt[np.maximum(si, 0)], -1)
            assert np.array_equal(back[unique[pq]], ri[pq][unique[pq]]), (nq, nt)
            assert unique.sum() > nq // 2
    if nq == 1 and nt == 1:                                       # the one query's coordinate NaN: nothing, not even at (1e6, 1e6)
        bad = np.array([[np.nan, 5.0]], np.float32)
        _compare(ctx, q, t, bad, xy_t0, (1e6, 1e6), "nan query", D)


def test_huge_window_equals_the_plain_kernel(ctx):
    """With finite coordinates a (1e6, 1e6) window masks nothing: the plain kernel's and the cross-check kernel's words exactly."""
    rng = np.random.default_rng(77)
    for nq, nt in SIZES:
        q, t, _, _ = _inputs(nq, nt, 2000 + nq + nt)
        xy_q = (rng.random((nq, 2)) * [640, 480]).astype(np.float32)
        xy_t = (rng.random((nt, 2)) * [640, 480]).astype(np.float32)
        pi, pd = ctx.bf_knn2(q, t)
        gi, gd = ctx.bf_knn2_window(q, t, xy_q, xy_t, (1e6, 1e6))
        assert np.array_equal(gi, pi) and np.array_equal(gd, pd), (nq, nt)
        mi, md, mm, mt = ctx.bf_knn2_mutual(q, t)
        xi, xd, xm, xt = ctx.bf_knn2_window(q, t, xy_q, xy_t, (1e6, 1e6), cross_check=True)
        assert np.array_equal(xi, mi) and np.array_equal(xd, md) and np.array_equal(xm, mm) and np.array_equal(xt, mt), (nq, nt)


def test_window_flag_without_a_window_is_refused(oracle):
    c = _native.Context(0, 640, 480, 64, 600)
    try:
        m = ctypes.c_int(0)
        us = ctypes.c_double(0)
        for call in (lambda: c._lib.vo_point_clouds_ex(c._h, 0, 1, 0.8, _native.VO_MATCH_WINDOW, None, None, None, None, None, None, 0, ctypes.byref(m)),
                     lambda: c._lib.vo_measure_knn_ex(c._h, 0, 1, 5, _native.VO_MATCH_WINDOW | _native.VO_MATCH_CROSSCHECK, ctypes.byref(us)),
                     lambda: c._lib.vo_measure_knn_ex(c._h, 0, 1, 5, 4, ctypes.byref(us))):
            with pytest.raises(_native.VoError) as e:
                c._ck(call())
            assert e.value.code == -1, str(e.value)               # VO_E_ARG
        for bad in ((-1.0, 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
            assert c._lib.vo_set_match_window(c._h, *bad) == -1
        with pytest.raises(_native.VoError):                     # still none set
            c._ck(c._lib.vo_measure_knn_ex(c._h, 0, 1, 5, _native.VO_MATCH_WINDOW, ctypes.byref(us)))
        assert c._lib.vo_set_match_window(c._h, 8.0, 8.0) == 0 and c._lib.vo_clear_match_window(c._h) == 0
        with pytest.raises(_native.VoError):                     # cleared
            c._ck(c._lib.vo_measure_knn_ex(c._h, 0, 1, 5, _native.VO_MATCH_WINDOW, ctypes.byref(us)))
        rng = np.random.default_rng(4)
        q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (170, 32), dtype=np.uint8)
        gi, gd = c.bf_knn2(q, t)
        ri, rd = oracle.bf_knn2_hamming(q, t)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)
    finally:
        c.close()


# ---- the consumers ---------------------------------------------------------------------------------------------------------------
WIN = (24, 16)


class _CachedRefCamera:
    """RefStereoCamera whose (slow) per-frame result is shared by the oracle odometers of this module"""

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


def _window_matches(f1, f2, window, ratio, cross):
    """the match set (q, t) of two oracle frames: windowed kNN-2 -> ratio test (-> mutual within the window)"""
    xa, xb = f1["kps"]["xy"], f2["kps"]["xy"]
    if cross:
        idx, dist, mutual, _ = W.window_knn2_mutual(f1["desc"], f2["desc"], xa, xb, *window)
    else:
        idx, dist = W.window_knn2(f1["desc"], f2["desc"], xa, xb, *window)
    q, t = W.ratio_filter(idx, dist, ratio)
    if cross:
        keep = mutual[q] == 1
        q, t = q[keep], t[keep]
    return q, t


def _wref_class(window, cross=False):
    from oracle import oracle as O
    from oracle.odometer import RefStereoOdometer

    class WRefStereoOdometer(RefStereoOdometer):
        """RefStereoOdometer whose point_clouds matches inside the window, scaled by the frames the pair spans: skipped_frames + 1
        for (current, next), skipped_frames + 2 for the one-frame-back fallback"""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.log, self.fallbacks = [], 0         # per pair (span, matches, gained over the plain set, lost from it)

        def point_clouds(self, f1, f2):
            fallback = f1 is self.prev
            self.fallbacks += int(fallback)
            span = self.skipped_frames + (2 if fallback else 1)
            radii = tuple(np.float32(r * span) for r in window)
            q, t = _window_matches(f1, f2, radii, self.match_threshold, cross)
            pq, pt = O.ratio_filter(*O.bf_knn2_hamming(f1["desc"], f2["desc"]), self.match_threshold)
            a, b = set(zip(q.tolist(), t.tolist())), set(zip(pq.tolist(), pt.tolist()))
            self.log.append((span, len(q), len(a - b), len(b - a)))
            if len(q) < self.min_matches:
                return None, None
            p1, s1 = f1["d3"].sample(f1["kps"]["xy"][q])
            p2, s2 = f2["d3"].sample(f2["kps"]["xy"][t])
            if (s1 == 2).any() or (s2 == 2).any():
                raise ZeroDivisionError("division by zero")
            self.last_matches = (q, t)
            return p1, p2
    return WRefStereoOdometer


@pytest.fixture(scope="module")
def c1():
    from oracle.odometer import RefStereoCamera
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
    rcam = _CachedRefCamera(RefStereoCamera(cam.Q, cam.valid_region_left, c.sgbm_params()))
    return dict(c=c, cam=cam, rcam=rcam, frames=c.pairs(0, 8))


def _chain(odo, frames):
    return [(odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()) for L, R in frames]


def _same_chain(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[2] == w[2] and (g[0] or g[1] == w[1]), (what, k, g[:3], w[:3])
        assert np.allclose(g[3], w[3], rtol=0, atol=1e-9), (what, k)


def _end_point_error(odo, n):
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(n - 1)
    return float(np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3]))


@pytest.mark.parametrize("name,kw", [("default", {}), ("clique", dict(rigidity_threshold=0.1, outlier_threshold=0.02)),
                                     ("cross", dict(cross_check=True))])
def test_stereo_chain_with_a_match_window_through_update_and_run(c1, name, kw):
    """C1 frames 0-7 with match_window=(24, 16): decisions, skip_cause, skipped_frames, the match set of every pair and the
    chained pose (1e-9) equal the oracle odometer's with the helper as its matcher, through update() (the fused synchronous
    step) and through run(depth=4) (steps begun ahead, keyed by the radii).  On the default odometer the window brings the
    end-point error below half the plain chain's (CPU oracle: 0.104 m against 1.303 m)."""
    from oracle.odometer import RefStereoOdometer
    cam, rcam, frames = c1["cam"], c1["rcam"], c1["frames"]
    ctx = cam._ctx
    cross = bool(kw.get("cross_check"))
    rkw = {k: v for k, v in kw.items() if k != "cross_check"}
    rodo = _wref_class(WIN, cross)(rcam, preprocessed_frames=True, **rkw)
    want = _chain(rodo, frames)
    assert len(rodo.log) == len(frames) - 1 and all(g + l > 0 for _, _, g, l in rodo.log), rodo.log   # the window changes every pair's set
    assert all(span == 1 for span, _, _, _ in rodo.log)
    print("%s: matches / gained / lost per pair: %s" % (name, [x[1:] for x in rodo.log]))
    # update(): the fused synchronous step; the match set of every accepted pair
    odo = StereoOdometer(cam, preprocessed_frames=True, match_window=WIN, **kw)
    rodo2 = _wref_class(WIN, cross)(rcam, preprocessed_frames=True, **rkw)
    got = []
    for k, (L, R) in enumerate(frames):
        a, b = odo.update(L, R), rodo2.update(L, R)
        got.append((a, odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()))
        assert a == b and odo.skip_cause == rodo2.skip_cause, (name, k)
        if k and a and odo.prev_kps.frame.live and odo.current_kps.frame.live:
            sa, sb = odo.prev_kps.frame.slot, odo.current_kps.frame.slot
            counts = ctx.pose_pair(sa, sb, *odo._pose_params())[0]
            q, t = ctx.point_clouds(sa, sb, 0.8, cross, window=WIN)[:2]
            assert int(counts[0]) == len(rodo2.last_matches[0]) == len(q), (name, k)
            assert np.array_equal(q, rodo2.last_matches[0]) and np.array_equal(t, rodo2.last_matches[1]), (name, k)
    _same_chain(got, want, name + " update")
    # run(): steps begun ahead carry the radii in their key
    odo = StereoOdometer(cam, preprocessed_frames=True, match_window=WIN, **kw)
    got = [(ok, odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()) for ok in odo.run(iter(frames), depth=4)]
    _same_chain(got, want, name + " run")
    odo.reset_lookahead()
    # the plain chain: the oracle's, untouched by what ran before it on this camera -- and for the default odometer far worse
    plain = RefStereoOdometer(rcam, preprocessed_frames=True, **rkw)
    ref_plain = [(plain.update(L, R), plain.c_T_w.copy()) for L, R in frames]
    podo = StereoOdometer(cam, preprocessed_frames=True, **rkw)
    gotp = [(ok, podo.c_T_w.copy()) for ok in podo.run(iter(frames), depth=4)]
    for (ga, gT), (ra, rT) in zip(gotp, ref_plain):
        assert ga == ra and np.allclose(gT, rT, rtol=0, atol=1e-9)
    podo.reset_lookahead()
    e_win, e_plain = _end_point_error(rodo, len(frames)), _end_point_error(plain, len(frames))
    print("%s: end-point error %.3f m with the window, %.3f m without" % (name, e_win, e_plain))
    if name == "default":
        assert e_win < 0.5 * e_plain, (e_win, e_plain)
    assert ctx.sgbm_sweep_status() == 0


def test_fallback_pair_scales_the_window_with_its_span(c1):
    """C1 with frame 3 replaced by noise: (2, noise) fails, the one-frame-back fallback (1, noise) runs with twice the radii and
    fails too, the frame is skipped, and (2, 4) is matched with twice the radii: the GPU chain equals the windowed oracle's."""
    cam, rcam = c1["cam"], c1["rcam"]
    rng = np.random.default_rng(1)
    frames = list(c1["frames"][:7])
    shape = frames[3][0].shape
    frames[3] = (rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8))
    rodo = _wref_class(WIN)(rcam, preprocessed_frames=True)
    want = _chain(rodo, frames)
    assert rodo.fallbacks >= 1 and not all(w[0] for w in want), (rodo.fallbacks, [w[:3] for w in want])
    assert sorted(set(x[0] for x in rodo.log)) == [1, 2], rodo.log           # both spans occurred
    odo = StereoOdometer(cam, preprocessed_frames=True, match_window=WIN)
    _same_chain(_chain(odo, frames), want, "fallback update")
    odo = StereoOdometer(cam, preprocessed_frames=True, match_window=WIN)
    got = [(ok, odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()) for ok in odo.run(iter(frames), depth=4)]
    _same_chain(got, want, "fallback run")
    odo.reset_lookahead()


def test_pnp_with_a_match_window_fused_equals_composed_equals_the_helper(c1):
    """pose_method="pnp" with a window: the composed path's point_clouds receives the window and returns the helper's match
    set; the fused step (update() and run()) gives the composed path's chain exactly; with pnp_refine=3 the fused step still
    counts the helper's matches and refines the same winner."""
    cam, frames = c1["cam"], c1["frames"]
    ctx = cam._ctx
    kw = dict(preprocessed_frames=True, pose_method="pnp", match_window=WIN)
    comp = StereoOdometer(cam, **kw)
    comp._pnp_fused = False
    seen = []
    real = ctx.point_clouds

    def spy(sa, sb, ratio, cross_check=False, window=None):
        out = real(sa, sb, ratio, cross_check, window=window)
        ka, kb = ctx.download_keypoints(sa), ctx.download_keypoints(sb)
        q, t = _window_matches(dict(kps=ka, desc=ka["desc"]), dict(kps=kb, desc=kb["desc"]), window, ratio, cross_check)
        assert window == (24.0, 16.0) and np.array_equal(out[0], q) and np.array_equal(out[1], t)
        seen.append(len(q))
        return out
    ctx.point_clouds = spy
    try:
        want = _chain(comp, frames)
    finally:
        del ctx.point_clouds
    assert len(seen) == len(frames) - 1 and all(w[0] for w in want)
    fused = StereoOdometer(cam, **kw)
    got = _chain(fused, frames)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w[:3] and np.array_equal(g[3], w[3]), k
    sa, sb = fused.prev_kps.frame.slot, fused.current_kps.frame.slot
    K4 = fused._pose_params()[2]
    r0 = ctx.pnp_pair_window(sa, sb, 0.8, K4, WIN, want_matches=True)
    r3 = ctx.pnp_pair_window(sa, sb, 0.8, K4, WIN, refine=3, want_matches=True)
    assert r0["matches"] == r3["matches"] == seen[-1] and r3["refine_status"] == 0
    assert np.array_equal(r0["Rt"], r3["Rt"]) and np.array_equal(r0["mask"], r3["mask"]) and np.array_equal(r0["q"], r3["q"])
    assert r0["matches"] != ctx.pnp_pair(sa, sb, 0.8, K4)["matches"]                       # (the plain step is another set)
    tk = ctx.pnp_pair_begin_window(sa, sb, 0.8, K4, WIN, refine=3, want_matches=True)
    ctx.bf_knn2_window(np.zeros((1, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros((1, 2)), np.zeros((2, 2)), (1, 1))
    re = ctx.pnp_pair_end(tk, want_matches=True)
    assert re["matches"] == r3["matches"] and np.array_equal(re["Rt_refined"], r3["Rt_refined"]) and np.array_equal(re["mask"], r3["mask"])
    fused = StereoOdometer(cam, **kw)
    got = [(ok, fused.skip_cause, fused.skipped_frames, fused.c_T_w.copy()) for ok in fused.run(iter(frames), depth=4)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w[:3] and np.array_equal(g[3], w[3]), k
    fused.reset_lookahead()
    a = StereoOdometer(cam, pnp_refine=3, **kw)
    upd = _chain(a, frames)
    b = StereoOdometer(cam, pnp_refine=3, **kw)
    run = [(ok, b.skip_cause, b.skipped_frames, b.c_T_w.copy()) for ok in b.run(iter(frames), depth=4)]
    b.reset_lookahead()
    for k, (g, w) in enumerate(zip(run, upd)):
        assert g[:3] == w[:3] and np.array_equal(g[3], w[3]), k
    assert all(u[0] for u in upd) and not np.array_equal(upd[-1][3], want[-1][3])          # (the refinement does move the pose)


def test_mono_steps_with_a_match_window(oracle, c1):
    """mono_pair(window=...) at 640 x 480 with 1500 features, solvers 5 and 8, equals the oracle composition windowed kNN-2 ->
    ratio test -> ransac_essential (M, winner, inlier count, mask, q / t, E to 1e-12); begin / end gives the synchronous result;
    mono_pose_pair agrees on the shared fields; MonoOdometer(match_window=...) uses it."""
    from openvo_amd.mono import MonoOdometer
    c = c1["c"]
    frames = [c1["frames"][k][0] for k in (0, 1)]
    assert (c.w, c.h) == (640, 480)
    ctx = _native.Context(0, c.w, c.h, 64, 4200)
    try:
        for s, f in enumerate(frames):
            ctx.upload_mono(s, f)
            assert ctx.orb_slot_count(s, 1500, 0) > 1000
        K4 = [c.f, c.f, c.cx, c.cy]
        ref = [oracle.orb_detect_and_compute(f, None, 1500) for f in frames]
        fr = [dict(kps=r, desc=r["desc"]) for r in ref]
        rq, rt = _window_matches(fr[0], fr[1], WIN, 0.8, False)
        plain_m = len(oracle.ratio_filter(*oracle.bf_knn2_hamming(ref[0]["desc"], ref[1]["desc"]), 0.8)[0])
        assert len(rq) > 100 and len(rq) != plain_m
        for solver in (8, 5):
            got = ctx.mono_pair(0, 1, 0.8, K4, 2000, 1.0, 4321, want_matches=True, solver=solver, window=WIN)
            rr = oracle.ransac_essential(ref[0]["xy"][rq], ref[1]["xy"][rt], K4, 2000, 1.0, 4321, solver=solver)
            assert got["matches"] == len(rq) and np.array_equal(got["q"], rq) and np.array_equal(got["t"], rt)
            assert got["best_iter"] == rr["best_iter"] and got["best_count"] == rr["best_count"], solver
            assert np.array_equal(got["mask"], rr["mask"]) and np.allclose(got["E"], rr["E"], rtol=0, atol=1e-12)
            tk = ctx.mono_pair_begin(0, 1, 0.8, K4, 2000, 1.0, 4321, want_matches=True, solver=solver, window=WIN)
            ctx._mflags(False, (3, 3))                              # another window set meanwhile: the step keeps the one it was begun with
            ga = ctx.mono_pair_end(tk, want_matches=True)
            assert ga["matches"] == got["matches"] and ga["best_iter"] == got["best_iter"] and ga["best_count"] == got["best_count"]
            assert np.array_equal(ga["mask"], got["mask"]) and np.array_equal(ga["q"], got["q"]) and np.array_equal(ga["t"], got["t"])
            assert np.array_equal(ga["E"], got["E"])
            gp = ctx.mono_pose_pair(0, 1, 0.8, K4, 2000, 1.0, 4321, solver=solver, window=WIN)
            assert gp["matches"] == got["matches"] and gp["best_iter"] == got["best_iter"] and gp["best_count"] == got["best_count"]
            assert np.array_equal(np.asarray(gp["E"]).reshape(-1), np.asarray(got["E"]).reshape(-1))
            tk, _ = ctx.mono_pose_pair_begin(0, 1, 0.8, K4, 2000, 1.0, 4321, solver=solver, window=WIN)
            ge = ctx.mono_pose_pair_end(tk)
            assert ge["matches"] == gp["matches"] and ge["best_count"] == gp["best_count"] and np.array_equal(ge["E"], gp["E"])
            assert ctx.mono_pair(0, 1, 0.8, K4, 2000, 1.0, 4321, solver=solver)["matches"] == plain_m       # the default is untouched
        K = np.array([[c.f, 0, c.cx], [0, c.f, c.cy], [0, 0, 1.0]])
        for dev in (False, True):
            odo = MonoOdometer(K, (c.w, c.h), nfeatures=1500, context=ctx, match_window=WIN, pose_on_device=dev, ransac_iters=2000)
            for f in frames:
                assert odo.update(f), odo.skip_cause
            assert odo.last["matches"] == len(rq), dev
    finally:
        ctx.close()
