"""The fitting half of the fused pose step (pose_fit_block / dev_umeyama_block / dev_svd3 in csrc/geom.hip) restated in numpy IN
THE KERNEL'S OWN SUMMATION ORDER, for up to 1024 point pairs (the one-wave path): the composed path vo_rigid_clique -> vo_umeyama
sums in another order and agrees with the fused step only to the last bits; this one is meant to agree bit for bit.

    wave_sum(v)                  wave_sum_f64_dpp on 64 per-lane values: inclusive row scan by shifts 1, 2, 4, 8, then rows 1 and 3
                                 take lane 15 of the row before, rows 2 and 3 take lane 31; the result is lane 63
    umeyama(src, dst)            dev_umeyama_block (force_rotation): -> (T 3x4, scale, rc)
    pose_fit(pa, pb, outlier)    pose_fit_block on the points that survived the clique filter -> (n2, rc1, rc2, T2)

Float64 throughout on float32 inputs, no fused multiply-add, every sum in the order written; sqrt and division are correctly
rounded on both sides."""
import math

import numpy as np


def wave_sum(v):
    v = np.asarray(v, np.float64).copy()
    assert v.shape == (64,)
    for sh in (1, 2, 4, 8):
        t = np.zeros(64)
        for r in range(4):
            t[16 * r + sh:16 * r + 16] = v[16 * r:16 * r + 16 - sh]
        v = v + t
    t = np.zeros(64)
    t[16:32], t[48:64] = v[15], v[47]
    v = v + t
    t = np.zeros(64)
    t[32:64] = v[31]
    v = v + t
    return float(v[63])


def _lane_sums(terms):
    """terms: (n, k) float64, point i belongs to lane i % 64 and is added in ascending i -> k wave sums"""
    n, k = terms.shape
    acc = np.zeros((64, k))
    for i0 in range(0, n, 64):
        blk = terms[i0:i0 + 64]
        acc[:len(blk)] = acc[:len(blk)] + blk
    return [wave_sum(acc[:, c]) for c in range(k)]


def _rotate(G, V, P, Q):
    al = be = ga = 0.0
    for i in range(3):
        al += G[i][P] * G[i][P]
        be += G[i][Q] * G[i][Q]
        ga += G[i][P] * G[i][Q]
    if abs(ga) <= 1e-300 or abs(ga) <= 2.2204460492503131e-16 * math.sqrt(al * be):
        return False
    zeta = (be - al) / (2.0 * ga)
    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
    c = 1.0 / math.sqrt(1.0 + t * t)
    s = c * t
    for i in range(3):
        gp, gq = G[i][P], G[i][Q]
        G[i][P], G[i][Q] = c * gp - s * gq, s * gp + c * gq
        vp, vq = V[i][P], V[i][Q]
        V[i][P], V[i][Q] = c * vp - s * vq, s * vp + c * vq
    return True


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def svd3(A):
    """dev_svd3: one-sided Jacobi -> (U 3x3, w 3, Vt 3x3) as nested lists, singular values descending"""
    G = [[float(A[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(60):
        rot = _rotate(G, V, 0, 1)
        rot = _rotate(G, V, 0, 2) or rot
        rot = _rotate(G, V, 1, 2) or rot
        if not rot:
            break
    sv = [math.sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]) for j in range(3)]
    o = [0, 1, 2]
    if sv[o[1]] > sv[o[0]]:
        o[0], o[1] = o[1], o[0]
    if sv[o[2]] > sv[o[0]]:
        o[0], o[2] = o[2], o[0]
    if sv[o[2]] > sv[o[1]]:
        o[1], o[2] = o[2], o[1]
    w = [sv[k] for k in o]
    Vc = [[V[i][k] for i in range(3)] for k in o]
    Uc = [[(G[i][k] / sv[k] if sv[k] > 0 else 0.0) for i in range(3)] for k in o]
    tiny = w[0] * 1e-300 + 1e-300
    if w[1] <= tiny:
        a = [0.0, 1.0, 0.0] if abs(Uc[0][0]) > 0.9 else [1.0, 0.0, 0.0]
        Uc[1] = _cross(Uc[0], a)
        nn = math.sqrt(Uc[1][0] * Uc[1][0] + Uc[1][1] * Uc[1][1] + Uc[1][2] * Uc[1][2])
        Uc[1] = [(x / nn if nn != 0 else math.nan) for x in Uc[1]]     # (a zero covariance: 0 / 0 on the device, then rc = -2)
    if w[2] <= tiny or w[2] <= 1e-14 * w[0]:
        Uc[2] = _cross(Uc[0], Uc[1])
        nn = math.sqrt(Uc[2][0] * Uc[2][0] + Uc[2][1] * Uc[2][1] + Uc[2][2] * Uc[2][2])
        if nn > 0:
            Uc[2] = [x / nn for x in Uc[2]]
    U = [[Uc[j][i] for j in range(3)] for i in range(3)]
    return U, w, Vc


def _det3(m):
    m = [x for row in m for x in row]
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def umeyama(src, dst, min_n=3):
    """-> (T 3x4 float64 or None, scale, rc): rc 0 ok, 1 not attempted, -1 fewer than 3 points, -2 colinear"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    n = len(src)
    assert n <= 1024, "the one-wave path only"
    if n < min_n or n < 3:
        return None, 0.0, (-1 if n < 3 else 1)
    s64, d64 = src.astype(np.float64), dst.astype(np.float64)
    a = _lane_sums(np.concatenate([s64, d64], axis=1))
    inv = 1.0 / n
    ms, md = [a[c] * inv for c in range(3)], [a[3 + c] * inv for c in range(3)]
    s, d = s64 - np.array(ms), d64 - np.array(md)
    terms = np.empty((n, 10))
    for r in range(3):
        for c in range(3):
            terms[:, r * 3 + c] = d[:, r] * s[:, c]
    terms[:, 9] = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    a = _lane_sums(terms)
    cov = [[a[r * 3 + c] * inv for c in range(3)] for r in range(3)]
    U, w, Vt = svd3(cov)
    if (w[0] != 0) + (w[1] != 0) + (w[2] != 0) < 2:
        return None, 0.0, -2
    S = [1.0, 1.0, -1.0 if _det3(U) * _det3(Vt) < 0 else 1.0]
    T = np.zeros((3, 4))
    R = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for k in range(3):
                acc += U[r][k] * S[k] * Vt[k][c]
            R[r][c] = acc
    sc = (w[0] * S[0] + w[1] * S[1] + w[2] * S[2]) * (float(n) / a[9])
    for r in range(3):
        nt = 0.0
        for c in range(3):
            T[r, c] = R[r][c]
            nt += R[r][c] * ms[c]
        T[r, 3] = md[r] - sc * nt
    return T, sc, 0


def pose_fit(pa, pb, outlier_thr, min_matches=10):
    """pa / pb: the n1 point pairs behind the clique filter (match order) -> (n2, rc1, rc2, T2 or None)"""
    pa, pb = np.asarray(pa, np.float32).reshape(-1, 3), np.asarray(pb, np.float32).reshape(-1, 3)
    n1, rc1 = len(pa), 1
    if outlier_thr > 0 and n1 >= 10:
        T, _, rc1 = umeyama(pa, pb)
        if rc1 == 0:
            x, y, z = (pa[:, c].astype(np.float64) for c in range(3))
            X, Y, Z = (pb[:, c].astype(np.float64) for c in range(3))
            r = [((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)]
            dx, dy, dz = X - r[0], Y - r[1], Z - r[2]
            dw = 1.0 - (((0.0 * x + 0.0 * y) + 0.0 * z) + 1.0)
            e = np.sqrt(((dx * dx + dy * dy) + dz * dz) + dw * dw) / np.sqrt(((X * X + Y * Y) + Z * Z) + 1.0)
            if np.isnan(e).any():
                keep = np.zeros(n1, bool)
            else:
                order = np.argsort(e, kind="stable")          # rank by (value, index)
                med = 0.5 * e[order[n1 // 2]] + 0.5 * e[order[(n1 - 1) // 2]]
                keep = e < outlier_thr + med
            pa, pb = pa[keep], pb[keep]
    n2 = len(pa)
    if n2 < min_matches:
        return n2, rc1, 1, None
    T2, _, rc2 = umeyama(pa, pb)
    return n2, rc1, rc2, T2
