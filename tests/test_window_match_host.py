"""Windowed matching (Hamming kNN-2 inside a pixel window), the host side: the numpy restatement the GPU tests hold the kernel
against is itself held against hand-written answers and the oracle; the odometers validate match_window, scale it with the
frame span and key their steps begun ahead by the effective radii; the library exports the new entries."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_match_ref as W  # noqa: E402

N, INF = W.NONE_IDX, W.NONE_DIST


def _desc(bits):
    """a descriptor with the first `bits` bits set: the distance between two of them is the difference of their counts"""
    d = np.zeros(256, np.uint8)
    d[:bits] = 1
    return np.packbits(d)


def test_helper_against_hand_written_answers():
    #            query 0: a tie broken by the index, query 1: exactly one candidate, query 2: none,
    #            query 3: radius-0 hit on one axis (dy = 0 exactly, ry = 0) and a NaN train beside it
    q = np.stack([_desc(10), _desc(20), _desc(30), _desc(40)])
    t = np.stack([_desc(13), _desc(7), _desc(12), _desc(21), _desc(40), _desc(44)])
    xy_q = np.array([[100, 100], [200, 100], [300, 300], [50, 400]], np.float32)
    xy_t = np.array([[104, 100],      # in q0's window, distance 3
                     [96, 100],       # in q0's window, distance 3: the tie, index 1 loses to index 0
                     [100.5, 100],    # in q0's window, distance 2: the best
                     [195, 100],      # q1's only candidate, distance 1
                     [np.nan, 400],   # distance 0 to q3 but in no window
                     [55, 400]], np.float32)    # q3: |dx| = 5 = rx exactly, dy = 0 = ry
    idx, dist = W.window_knn2(q, t, xy_q, xy_t, 5.0, 0.0)
    assert idx.tolist() == [[2, 0], [3, N], [N, N], [5, N]]
    assert dist.tolist() == [[2, 3], [1, INF], [INF, INF], [4, INF]]
    assert idx.dtype == np.int32 and dist.dtype == np.int32
    # the same with the cross-check: a(j) over the queries that have j in their window
    idx2, dist2, mutual, t_best = W.window_knn2_mutual(q, t, xy_q, xy_t, 5.0, 0.0)
    assert np.array_equal(idx2, idx) and np.array_equal(dist2, dist)
    assert t_best.tolist() == [[0, 3], [0, 3], [0, 2], [1, 1], [N, INF], [3, 4]]
    assert mutual.tolist() == [1, 1, 0, 1]
    # a radius of 0 on both axes: equal positions only
    xy_t0 = xy_t.copy()
    xy_t0[1] = xy_q[0]
    idx, dist = W.window_knn2(q, t, xy_q, xy_t0, 0.0, 0.0)
    assert idx.tolist() == [[1, N], [N, N], [N, N], [N, N]] and dist[0].tolist() == [3, INF]
    # one step past the radius is out
    xy_t1 = xy_t.copy()
    xy_t1[5, 0] = np.nextafter(np.float32(55), np.float32(np.inf))
    assert W.window_knn2(q, t, xy_q, xy_t1, 5.0, 0.0)[0][3].tolist() == [N, N]
    # a NaN QUERY coordinate: no candidates at all
    xy_qn = xy_q.copy()
    xy_qn[0, 1] = np.nan
    assert W.window_knn2(q, t, xy_qn, xy_t, 1e6, 1e6)[0][0].tolist() == [N, N]
    # the ratio test: a query without a second neighbour gives no match
    qq, tt = W.ratio_filter(*W.window_knn2(q, t, xy_q, xy_t, 5.0, 0.0), 0.8)
    assert qq.tolist() == [0] and tt.tolist() == [2]


def test_helper_with_a_huge_window_equals_the_oracle(oracle):
    rng = np.random.default_rng(5)
    for nq, nt in ((70, 33), (3, 1), (200, 515)):
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        if nt > 9:
            t[7] = t[2]; q[1] = t[2]; q[4] = q[1]
        xy_q = (rng.random((nq, 2)) * 600).astype(np.float32)
        xy_t = (rng.random((nt, 2)) * 600).astype(np.float32)
        idx, dist, mutual, t_best = W.window_knn2_mutual(q, t, xy_q, xy_t, 1e6, 1e6)
        ri, rd = oracle.bf_knn2_hamming(q, t)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd), (nq, nt)
        bi, bd = oracle.bf_knn2_hamming(t, q)
        assert np.array_equal(t_best[:, 0], bi[:, 0]) and np.array_equal(t_best[:, 1], bd[:, 0])
        if nt >= 2:
            a, b = W.ratio_filter(idx, dist, 0.8), oracle.ratio_filter(ri, rd, 0.8)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_odometers_validate_match_window():
    from openvo_amd import StereoOdometer
    from openvo_amd.mono import MonoOdometer
    for bad in (-1, (3, -1), (1, 2, 3), "wide", (float("nan"), 2), float("inf"), (1, float("inf")), True, [], (None, 2), 1e39):
        with pytest.raises(ValueError):
            StereoOdometer(None, match_window=bad)
        with pytest.raises(ValueError):
            MonoOdometer(np.eye(3), (64, 64), match_window=bad, context=object())
    assert StereoOdometer(None).match_window is None
    assert StereoOdometer(None, match_window=24).match_window == (24.0, 24.0)
    assert StereoOdometer(None, match_window=(24, 16)).match_window == (24.0, 16.0)
    assert StereoOdometer(None, match_window=[0, 0.5]).match_window == (0.0, 0.5)
    assert StereoOdometer(None, match_window=np.array([3.0, 4.0])).match_window == (3.0, 4.0)
    assert MonoOdometer(np.eye(3), (64, 64), match_window=(8, 6), context=object()).match_window == (8.0, 6.0)
    # the radii are the float32 values the kernel compares with
    assert StereoOdometer(None, match_window=0.1).match_window == (float(np.float32(0.1)),) * 2


def test_pose_params_carry_the_radii_scaled_by_the_span():
    from openvo_amd import StereoOdometer
    plain = StereoOdometer(None)
    a, b = StereoOdometer(None, match_window=(24, 16)), StereoOdometer(None, match_window=(32, 24))
    assert plain._pose_params() == (0.8, 10, 0.0, 0.0, False)                      # without a window: what it was
    assert a._pose_params() == (0.8, 10, 0.0, 0.0, False, (24.0, 16.0))            # x 1
    assert a._pose_params() != b._pose_params() and a._pose_params()[:5] == b._pose_params()[:5]
    a.skipped_frames = 2
    assert a._pose_params()[-1] == (72.0, 48.0)                                    # x (skipped_frames + 1)
    assert a._window(span=4) == (96.0, 64.0)                                       # the fallback of that state: skipped_frames + 2
    a.skipped_frames = 0
    # _try_pair takes the span and hands it to whatever computes the pair
    seen = []
    a._try_pair_span = lambda *args: seen.append(a._pose_params()[-1])
    a._try_pair(*[None] * 6, span=3)
    a._try_pair(*[None] * 6)
    assert seen == [(72.0, 48.0), (24.0, 16.0)] and a._pair_span is None
    # update() passes skipped_frames + 1 for (current, next) and skipped_frames + 2 for the one-frame-back fallback
    spans = []

    class _Orb:
        def detectAndCompute(self, img, mask):
            return [None] * 50, "desc"

    class _Cam:
        def compute_3d(self, L, R, preprocessed=False):
            return "3d", np.zeros((2, 2), np.float32), "img"
    o = StereoOdometer(_Cam(), match_window=(24, 16))
    o.orb = _Orb()
    o._start_next_pose = lambda: None
    o._try_pair = lambda *args, span=None: (spans.append(span), np.eye(4) if len(spans) < 2 else None)[1]
    for _ in range(4):
        o.update(None, None)
    assert spans == [1, 1, 2, 2, 3]         # frame 1 accepted; frame 2: (cur, next) span 1, fallback span 2; frame 3: spans 2, 3
    pnp = StereoOdometer(None, pose_method="pnp", match_window=(8, 8))
    pnp.stereo = type("S", (), {"Q": np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 500.0], [0, 0, 1, 0]])})()
    assert pnp._pose_params()[-1] == (8.0, 8.0) and StereoOdometer._pnp_kwargs(pnp._pose_params())["window"] == (8.0, 8.0)


def test_generic_path_needs_a_windowed_matcher():
    from openvo_amd import StereoOdometer
    o = StereoOdometer(None, match_window=(24, 16))
    o.matcher = type("M", (), {"knnMatch": lambda self, a, b, k=2: ()})()
    with pytest.raises(ValueError):
        o.point_clouds([], [], None, None, None, None)


class _WinStub:
    """the native windowed call restated on the host"""

    def bf_knn2_window(self, q, t, xy_q, xy_t, window, cross_check=False):
        out = (W.window_knn2_mutual if cross_check else W.window_knn2)(q, t, xy_q, xy_t, *window)
        return out


def test_matcher_object_knn_match_window_shapes():
    from openvo_amd.features import BFMatcher
    q = np.stack([_desc(10), _desc(20), _desc(30), _desc(40)])
    t = np.stack([_desc(13), _desc(7), _desc(12), _desc(21), _desc(40), _desc(44)])
    xy_q = np.array([[100, 100], [200, 100], [300, 300], [50, 400]], np.float32)
    xy_t = np.array([[104, 100], [96, 100], [100.5, 100], [195, 100], [np.nan, 400], [55, 400]], np.float32)
    m = BFMatcher(_WinStub())
    got = m.knnMatchWindow(q, t, xy_q, xy_t, (5.0, 0.0), k=2)
    assert [[(d.queryIdx, d.trainIdx, d.distance) for d in row] for row in got] == \
        [[(0, 2, 2.0), (0, 0, 3.0)], [(1, 3, 1.0)], [], [(3, 5, 4.0)]]
    assert [len(r) for r in m.knnMatchWindow(q, t, xy_q, xy_t, (5.0, 0.0), k=1)] == [1, 1, 0, 1]
    kp = [type("KP", (), {"pt": (float(x), float(y))})() for x, y in xy_q]          # cv2-style keypoints work too
    assert [len(r) for r in m.knnMatchWindow(q, t, kp, xy_t, (5.0, 0.0))] == [2, 1, 0, 1]
    x = BFMatcher(_WinStub(), crossCheck=True)
    with pytest.raises(ValueError):
        x.knnMatchWindow(q, t, xy_q, xy_t, (5.0, 0.0), k=2)
    assert [len(r) for r in x.knnMatchWindow(q, t, xy_q, xy_t, (5.0, 0.0), k=1)] == [1, 1, 0, 1]
    with pytest.raises(ValueError):
        m.knnMatchWindow(q, t, xy_q[:3], xy_t, (5.0, 0.0))


def test_library_exports_the_window_entries():
    from openvo_amd import _native
    _native.build_native()
    lib = _native.lib()
    for name in ("vo_set_match_window", "vo_clear_match_window", "vo_bf_knn2_hamming_window"):
        assert name in _native.SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vo355.h")).read()
    assert "#define VO_MATCH_WINDOW 2" in header and _native.VO_MATCH_WINDOW == 2
    # hostile arguments give a status, not a crash (no context needed to refuse a NULL one)
    assert lib.vo_set_match_window(None, ctypes.c_float(1.0), ctypes.c_float(1.0)) != 0
    assert lib.vo_clear_match_window(None) != 0
    assert lib.vo_bf_knn2_hamming_window(None, None, 5, None, 5, None, None, ctypes.c_float(1.0), ctypes.c_float(1.0), 2,
                                         None, None, None, None) != 0
