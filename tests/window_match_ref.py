"""Windowed Hamming kNN-2 restated in numpy: the reference the window tests hold the kernel against (include/vo355.h).

Train j is a candidate of query i iff |xq_i - xt_j| <= rx and |yq_i - yt_j| <= ry, differences and comparisons in float32, a
NaN coordinate in no window.  Per query the two lexicographically smallest (distance, train index) among its candidates,
{-1, 0x7FFFFFFF} where they are missing.  Distances are an exact integer product of the unpacked bits."""
import numpy as np

NONE_IDX, NONE_DIST = -1, 0x7FFFFFFF


def hamming_table(q, t):
    """nq x nt int64 Hamming distances: |q| + |t| - 2 q.t on the unpacked bits (a float32 product of {0, 1} vectors of length
    256 is exact: every partial sum is an integer <= 256 < 2^24)"""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    qb = np.unpackbits(q, axis=1).astype(np.float32)
    tb = np.unpackbits(t, axis=1).astype(np.float32)
    dot = (qb @ tb.T).astype(np.int64)
    return qb.sum(1).astype(np.int64)[:, None] + tb.sum(1).astype(np.int64)[None, :] - 2 * dot


def window_mask(xy_q, xy_t, rx, ry):
    """nq x nt bool: train j in the window of query i (float32 arithmetic; NaN compares false)"""
    xy_q = np.asarray(xy_q, np.float32).reshape(-1, 2)
    xy_t = np.asarray(xy_t, np.float32).reshape(-1, 2)
    rx, ry = np.float32(rx), np.float32(ry)
    with np.errstate(invalid="ignore"):
        dx = np.abs(xy_q[:, None, 0] - xy_t[None, :, 0])
        dy = np.abs(xy_q[:, None, 1] - xy_t[None, :, 1])
        assert dx.dtype == np.float32 and dy.dtype == np.float32
        return (dx <= rx) & (dy <= ry)


def _two_smallest(D, mask):
    """per row of D the two smallest (value, column) keys among the masked columns -> (idx n x 2, dist n x 2)"""
    n, m = D.shape
    big = np.int64(1) << 40
    idx = np.full((n, 2), NONE_IDX, np.int32)
    dist = np.full((n, 2), NONE_DIST, np.int32)
    if m == 0 or n == 0:
        return idx, dist
    key = np.where(mask, D * 65536 + np.arange(m, dtype=np.int64)[None, :], big)      # (distance, index) in one integer: all distinct
    rows = np.arange(n)
    for k in range(2):
        col = key.argmin(axis=1)
        best = key[rows, col]
        has = best < big
        idx[has, k] = col[has].astype(np.int32)
        dist[has, k] = (best[has] >> 16).astype(np.int32)
        key[rows, col] = big
    return idx, dist


def window_knn2(q, t, xy_q, xy_t, rx, ry, table=None):
    """-> (idx nq x 2 int32, dist nq x 2 int32); table: hamming_table(q, t) when the caller already has it"""
    return _two_smallest(hamming_table(q, t) if table is None else table, window_mask(xy_q, xy_t, rx, ry))


def window_knn2_mutual(q, t, xy_q, xy_t, rx, ry, table=None):
    """-> (idx, dist, mutual nq uint8, t_best nt x 2 int32): a(j) = the smallest (distance, query index) over the queries that
    have j in their window; query i is mutual iff its best train b(i) exists and a(b(i)) == i"""
    D, mask = hamming_table(q, t) if table is None else table, window_mask(xy_q, xy_t, rx, ry)
    idx, dist = _two_smallest(D, mask)
    bi, bd = _two_smallest(D.T, mask.T)
    t_best = np.stack([bi[:, 0], bd[:, 0]], 1).astype(np.int32)
    b = idx[:, 0]
    mutual = np.array([b[i] >= 0 and t_best[b[i], 0] == i for i in range(len(b))], np.uint8)
    return idx, dist, mutual, t_best


def ratio_filter(idx, dist, ratio):
    """the ratio test on float32 distances in double (stereo_odometer.py:164); a query without two neighbours gives no match"""
    ok = idx[:, 1] >= 0
    d0 = dist[:, 0].astype(np.float32).astype(np.float64)
    d1 = dist[:, 1].astype(np.float32).astype(np.float64)
    keep = ok & (d0 < float(ratio) * d1)
    q = np.nonzero(keep)[0].astype(np.int32)
    return q, idx[keep, 0].astype(np.int32)
