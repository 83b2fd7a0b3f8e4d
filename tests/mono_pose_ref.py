"""numpy restatement of vo_recover_pose (include/vo355.h): the same arithmetic, sequentially and in the same order of operations
(float64, no fused multiply-add, three-term sums left to right), so that the device's doubles can be held to 1e-12 relative.

    decompose(E)                      -> R1, R2, t        one-sided Jacobi SVD as rs_svd3 (csrc/ransac.hip), det U, det Vt > 0
    depths(R, t, x1, x2)              -> z1, z2, sin2     per correspondence
    vote(R1, R2, t, x1, x2, inl)      -> votes4, winner
    depths_and_scale(R, t, ...)       -> dict             valid set, depth_b, z1, z2, n_depth, n_shared, scale_rel for a GIVEN pose
    recover_pose(E, ...)              -> dict             all of it: what vo_recover_pose returns
"""
import math

import numpy as np


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def svd3(A):
    """U, w, Vt of a 3x3 matrix: rs_svd3 operation for operation, in Python floats."""
    G = [float(v) for v in np.asarray(A, np.float64).reshape(9)]
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(60):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                al = be = ga = 0.0
                for i in range(3):
                    al += G[i * 3 + p] * G[i * 3 + p]
                    be += G[i * 3 + q] * G[i * 3 + q]
                    ga += G[i * 3 + p] * G[i * 3 + q]
                if abs(ga) <= 1e-300 or abs(ga) <= 2.2204460492503131e-16 * math.sqrt(al * be):
                    continue
                rotated = True
                zeta = (be - al) / (2.0 * ga)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for i in range(3):
                    gp, gq = G[i * 3 + p], G[i * 3 + q]
                    G[i * 3 + p] = c * gp - s * gq
                    G[i * 3 + q] = s * gp + c * gq
                    vp, vq = V[i * 3 + p], V[i * 3 + q]
                    V[i * 3 + p] = c * vp - s * vq
                    V[i * 3 + q] = s * vp + c * vq
        if not rotated:
            break
    sv = [math.sqrt(G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j]) for j in range(3)]
    order = [0, 1, 2]
    for i in range(2):
        for j in range(i + 1, 3):
            if sv[order[j]] > sv[order[i]]:
                order[i], order[j] = order[j], order[i]
    w = [sv[o] for o in order]
    Vc = [[V[i * 3 + o] for i in range(3)] for o in order]
    Uc = [[(G[i * 3 + o] / sv[o] if sv[o] > 0 else 0.0) for i in range(3)] for o in order]
    tiny = w[0] * 1e-300 + 1e-300
    if w[1] <= tiny:
        a = [1.0, 0.0, 0.0]
        if abs(Uc[0][0]) > 0.9:
            a = [0.0, 1.0, 0.0]
        Uc[1] = _cross(Uc[0], a)
        nn = math.sqrt(Uc[1][0] * Uc[1][0] + Uc[1][1] * Uc[1][1] + Uc[1][2] * Uc[1][2])
        with np.errstate(all="ignore"):               # (a zero E: 0 / 0 = NaN as on the device, where Python's floats would raise)
            Uc[1] = [float(np.float64(v) / np.float64(nn)) for v in Uc[1]]
    if w[2] <= tiny or w[2] <= 1e-14 * w[0]:
        Uc[2] = _cross(Uc[0], Uc[1])
        nn = math.sqrt(Uc[2][0] * Uc[2][0] + Uc[2][1] * Uc[2][1] + Uc[2][2] * Uc[2][2])
        if nn > 0:
            Uc[2] = [v / nn for v in Uc[2]]
    U = np.array(Uc, np.float64).T.copy()          # columns
    Vt = np.array(Vc, np.float64)
    return U, np.array(w), Vt


def _det3(M):
    M = [float(v) for v in np.asarray(M).reshape(9)]
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6])


def decompose(E):
    """R1 = U W Vt, R2 = U W^T Vt, t = U[:, 2] with det U, det Vt > 0 (the device's order of operations)."""
    U, _, Vt = svd3(E)
    if _det3(U) < 0.0:
        U = -U
    if _det3(Vt) < 0.0:
        Vt = -Vt
    R1, R2, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    for r in range(3):
        w0, w1, w2 = float(U[r, 1]), -float(U[r, 0]), float(U[r, 2])         # U W = [u1, -u0, u2]
        for c in range(3):
            R1[r, c] = (w0 * float(Vt[0, c]) + w1 * float(Vt[1, c])) + w2 * float(Vt[2, c])
            R2[r, c] = ((-w0) * float(Vt[0, c]) + (-w1) * float(Vt[1, c])) + w2 * float(Vt[2, c])
        t[r] = w2
    return R1, R2, t


def normalise(pts, K4):
    """float32 pixels -> float64 normalised points (K4 None: `pts` are normalised float64 points already)"""
    if K4 is None:
        return np.asarray(pts, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = [float(v) for v in K4]
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], 1)


def depths(R, t, x1, x2):
    """z1, z2, sin2 of every correspondence: z1 (R h1) + t = z2 h2."""
    R = np.asarray(R, np.float64)
    t0, t1, t2 = [float(v) for v in t]
    X1, Y1, hx, hy = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    ax = (R[0, 0] * X1 + R[0, 1] * Y1) + R[0, 2]
    ay = (R[1, 0] * X1 + R[1, 1] * Y1) + R[1, 2]
    az = (R[2, 0] * X1 + R[2, 1] * Y1) + R[2, 2]
    nx, ny, nz = hy * t2 - t1, t0 - hx * t2, hx * t1 - hy * t0
    dx, dy, dz = ay - az * hy, az * hx - ax, ax * hy - ay * hx
    dd = (dx * dx + dy * dy) + dz * dz
    hh = (hx * hx + hy * hy) + 1.0
    with np.errstate(all="ignore"):
        z1 = ((nx * dx + ny * dy) + nz * dz) / np.where(dd > 1e-300, dd, 1e-300)
        z2 = (((z1 * ax + t0) * hx + (z1 * ay + t1) * hy) + (z1 * az + t2)) / hh
        sin2 = dd / (((ax * ax + ay * ay) + az * az) * hh)
    return z1, z2, sin2


def vote(R1, R2, t, x1, x2, inl):
    """votes4 = (plus_1, minus_1, plus_2, minus_2) over the inliers; the winner: the largest vote, on a tie the rotation with the
    larger trace, then the lower index."""
    v = []
    for R in (R1, R2):
        z1, z2, _ = depths(R, t, x1, x2)
        v += [int(np.count_nonzero(inl & (z1 > 0) & (z2 > 0))), int(np.count_nonzero(inl & (z1 < 0) & (z2 < 0)))]
    tr1 = (float(R1[0, 0]) + float(R1[1, 1])) + float(R1[2, 2])
    tr2 = (float(R2[0, 0]) + float(R2[1, 1])) + float(R2[2, 2])
    best, bv, bt = 0, v[0], tr1
    if v[1] > bv:
        best, bv = 1, v[1]
    if v[2] > bv or (v[2] == bv and tr2 > bt):
        best, bv, bt = 2, v[2], tr2
    if v[3] > bv or (v[3] == bv and tr2 > bt):
        best, bv, bt = 3, v[3], tr2
    return np.array(v, np.int32), best


def lower_median(r):
    """the element of rank (n - 1) // 2 in ascending order; 0 for none"""
    r = np.sort(np.asarray(r, np.float64))
    return float(r[(len(r) - 1) // 2]) if len(r) else 0.0


def depths_and_scale(R, t, pts1, pts2, K4, mask=None, q_idx=None, t_idx=None, na=None, nb=None, depth_a=None, gate=0.0):
    """Everything behind the vote, for a GIVEN pose (R, signed t)."""
    x1, x2 = normalise(pts1, K4), normalise(pts2, K4)
    n = len(x1)
    inl = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if q_idx is None:
        q_idx = t_idx = np.arange(n)
        na = nb = n
    z1, z2, sin2 = depths(R, t, x1, x2)
    with np.errstate(invalid="ignore"):
        valid = inl & (z1 > 0) & (z2 > 0) & (sin2 >= gate)
    depth_b = np.zeros(nb)
    owned = np.zeros(nb, bool)
    for i in np.nonzero(valid)[0]:                    # ascending: the lowest i that names a keypoint wins
        if not owned[t_idx[i]]:
            owned[t_idx[i]] = True
            depth_b[t_idx[i]] = z2[i]
    ratios = []
    if depth_a is not None:
        d = np.asarray(depth_a, np.float64)[q_idx]
        with np.errstate(all="ignore"):
            shared = valid & (d > 0) & np.isfinite(d)
            ratios = (d / z1)[shared]
    return dict(valid=valid, depth_b=depth_b, z1=np.where(inl, z1, 0.0), z2=np.where(inl, z2, 0.0), n_depth=int(valid.sum()),
                n_shared=len(ratios), scale_rel=lower_median(ratios), ratios=np.asarray(ratios))


def recover_pose(E, pts1, pts2, K4, mask=None, q_idx=None, t_idx=None, na=None, nb=None, depth_a=None, gate=0.0):
    """What vo_recover_pose returns (flags, R, t, votes4, winner and the dict of depths_and_scale)."""
    n = len(np.asarray(pts1).reshape(-1, 2))
    inl = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    flags = 0 if depth_a is not None else 4
    if q_idx is not None:
        q_idx, t_idx = np.asarray(q_idx), np.asarray(t_idx)
        if (q_idx < 0).any() or (q_idx >= na).any() or (t_idx < 0).any() or (t_idx >= nb).any():
            flags |= 2
    else:
        na = nb = n
    R1, R2, t = decompose(E)
    if not inl.any() or not (np.isfinite(R1).all() and np.isfinite(R2).all() and np.isfinite(t).all()):
        flags |= 1
    if flags & 3:
        return dict(flags=flags, R=np.eye(3), t=np.zeros(3), votes4=np.zeros(4, np.int32), winner=0, valid=np.zeros(n, bool),
                    depth_b=np.zeros(nb), z1=np.zeros(n), z2=np.zeros(n), n_depth=0, n_shared=0, scale_rel=0.0)
    x1, x2 = normalise(pts1, K4), normalise(pts2, K4)
    votes4, winner = vote(R1, R2, t, x1, x2, inl)
    R, tw = (R1, R2)[winner >> 1], (t if (winner & 1) == 0 else -t)
    out = depths_and_scale(R, tw, pts1, pts2, K4, mask, q_idx, t_idx, na, nb, depth_a, gate)
    out.update(flags=flags, R=R, t=tw, votes4=votes4, winner=winner)
    return out
