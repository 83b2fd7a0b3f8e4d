"""Cross-check matching (mutual nearest neighbours): the host side, no GPU needed -- the cv2 slice accepts crossCheck=True and
mirrors OpenCV's refusal of k = 2, the odometers validate the option and key their steps begun ahead by it, and the matcher
object turns the native result into cv2's shapes.  Wherever a cv2 is importable, the semantics written into include/vo355.h
(mutual nearest neighbour, ties to the lower index both ways) are pinned against cv2.BFMatcher(NORM_HAMMING, crossCheck=True)."""
import numpy as np
import pytest

from openvo_amd import cv2_compat
from openvo_amd.features import BFMatcher


def _mutual_numpy(q, t):
    """independent restatement: popcount table, argmin (first = lower index) in both directions"""
    pc = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    D = pc[q[:, None, :] ^ t[None, :, :]].sum(-1)
    b = D.argmin(1)
    a = D.argmin(0)
    return b, D[np.arange(len(q)), b], a[b] == np.arange(len(q))


class _CtxStub:
    """the two native calls the matcher makes, restated on the host"""

    def bf_knn2(self, q, t):
        pc = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
        D = pc[q[:, None, :] ^ t[None, :, :]].sum(-1)
        o = np.argsort(D, axis=1, kind="stable")[:, :2]
        return o.astype(np.int32), np.take_along_axis(D, o, 1).astype(np.int32)

    def bf_knn2_mutual(self, q, t):
        idx, dist = self.bf_knn2(q, t)
        b, _, m = _mutual_numpy(q, t)
        return idx, dist, m.astype(np.uint8), None


def test_cv2_compat_bfmatcher_accepts_cross_check_and_refuses_k2():
    m = cv2_compat.BFMatcher.create(cv2_compat.NORM_HAMMING, crossCheck=True)
    assert m.crossCheck and callable(m.match)
    d = np.zeros((4, 32), np.uint8)
    with pytest.raises(cv2_compat.error):
        m.knnMatch(d, d, k=2)
    with pytest.raises(cv2_compat.error):
        cv2_compat.BFMatcher(cv2_compat.NORM_HAMMING + 1, crossCheck=True)
    assert not cv2_compat.BFMatcher(cv2_compat.NORM_HAMMING).crossCheck


def test_matcher_object_shapes_match_and_knn1():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (25, 32), dtype=np.uint8)
    q[7] = q[3]                                                  # two queries with one nearest train: one of them fails
    b, d, mut = _mutual_numpy(q, t)
    assert not mut.all()
    x = BFMatcher(_CtxStub(), crossCheck=True)
    got = x.match(q, t)
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(i, int(b[i]), float(d[i])) for i in range(len(q)) if mut[i]]
    k1 = x.knnMatch(q, t, k=1)
    assert len(k1) == len(q) and all((len(k1[i]) == 1) == bool(mut[i]) for i in range(len(q)))
    with pytest.raises(ValueError):
        x.knnMatch(q, t, k=2)
    plain = BFMatcher(_CtxStub())
    assert [(m.queryIdx, m.trainIdx) for m in plain.match(q, t)] == [(i, int(b[i])) for i in range(len(q))]
    assert [len(r) for r in plain.knnMatch(q, t, k=1)] == [1] * len(q)
    assert [len(r) for r in plain.knnMatch(q, t, k=2)] == [2] * len(q)


def test_odometers_validate_cross_check_and_key_their_steps_by_it():
    from openvo_amd import StereoOdometer
    from openvo_amd.mono import MonoOdometer
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError):
            StereoOdometer(None, cross_check=bad)
        with pytest.raises(ValueError):
            MonoOdometer(np.eye(3), (64, 64), cross_check=bad)
    a, b = StereoOdometer(None), StereoOdometer(None, cross_check=True)
    assert a.cross_check is False and b.cross_check is True
    assert a._pose_params() != b._pose_params() and a._pose_params()[:4] == b._pose_params()[:4]


def test_semantics_equal_cv2_cross_check():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    for nq, nt in ((200, 150), (60, 300), (1, 5)):
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        if nq > 10:
            q[5] = q[2]; t[3] = t[1]; q[8] = t[1]
        b, d, mut = _mutual_numpy(q, t)
        ref = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match(q, t)
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in ref] == [(i, int(b[i]), float(d[i])) for i in range(nq) if mut[i]]


@pytest.mark.gpu
def test_hip_match_equals_cv2_cross_check():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(12)
    for nq, nt in ((500, 450), (70, 900), (1, 3)):
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        if nq > 10:
            q[5] = q[2]; t[3] = t[1]; q[8] = t[1]
        ref = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match(q, t)
        got = cv2_compat.BFMatcher.create(cv2_compat.NORM_HAMMING, crossCheck=True).match(q, t)
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(m.queryIdx, m.trainIdx, m.distance) for m in ref]
