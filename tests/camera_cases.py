"""Generic cameras and the cameras a slip would produce: test infrastructure (numpy only).

Every camera-consuming kernel behind the fused steps was only ever run on a camera with fx == fy (and mostly the principal point at the
image centre), on which a kernel that reads fx for fy, cx for cy, the principal point from Q instead of K4, or Q[3][3] from another
(also zero) cell computes what its reference computes.  A GENERIC camera tells all of these apart:

    fx = 0.9 w, fy = 0.88 fx (12 % apart), (cx, cy) = (0.47 w + 0.3, 0.55 h - 0.2): cx != cy, neither at the image centre, neither
    an integer, and none of the four equal to a constant of the suites the camera is used in (their focal lengths are 400, 500, 700,
    650 and 0.9 w of other sizes, their principal points (320, 240), (352, 256), (w - 1) / 2).

mutants(K4, w, h) are the cameras a slip would produce; tests/test_camera_axes_ref.py asserts, on the CPU, that the reference of every
case of tests/test_gpu_camera_axes.py moves by at least 1000 x the bar of a compared field under each of them -- which is what proves,
without touching a kernel, that the device test fails on the slip.

Rejected values.  A case that is not sensitive to a mutant is changed until it is, and what was rejected is written down here:
    cameras, seeds       none: the first camera and the first seed tried for every case was sensitive to every mutant
    direct alignment     image B rendered with K^-1 as the ray map: inconsistent with a Q whose focal length is fx alone, the fit
                         walks 0.29 m away (tests/direct_cases.py renders with ray_map(Q))
    dense lookups        a 7 x 5 field: a planted field is at least 16 x 16 (19 x 16 taken)
    KLT PnP pair         the dense arm: its points come from Q, which has one focal length, so that a shifted image is no rigid
                         motion under fx != fy and RANSAC finds no consensus; the sparse arm plants its cloud under K4"""
import numpy as np


def generic(w, h):
    """K4 = (fx, fy, cx, cy) of the generic camera of a w x h image"""
    fx = 0.9 * w
    return (fx, 0.88 * fx, 0.47 * w + 0.3, 0.55 * h - 0.2)


K_640 = generic(640, 480)                  # (576.0, 506.88, 301.1, 263.8)
K_704 = generic(704, 512)                  # (633.6, 557.568, 331.18, 281.4)


def matrix(K4):
    fx, fy, cx, cy = K4
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def mutants(K4, w, h):
    """[(name, K4')]: fx / fy swapped, cx / cy swapped, fy read as fx, the principal point taken for the image centre"""
    fx, fy, cx, cy = K4
    return [("fx<->fy", (fy, fx, cx, cy)), ("cx<->cy", (fx, fy, cy, cx)), ("fy:=fx", (fx, fx, cx, cy)), ("c:=centre", (fx, fy, w / 2.0, h / 2.0))]


# ---- the direct alignment's rig: a Q of the five entries the header reads, and a K4 whose principal point is NOT Q's -------------------
Q32, Q33, K_OFFSET = 4.0, 0.8, (1.75, -1.25)


def direct_rig(w, h):
    """(Q 4x4, K4) with fx != fy, K4's principal point != (-Q[0][3], -Q[1][3]), Q[3][2] and Q[3][3] != 0"""
    fx, fy, qx, qy = generic(w, h)
    Q = np.array([[1, 0, 0, -qx], [0, 1, 0, -qy], [0, 0, 0, fx], [0, 0, Q32, Q33]], np.float64)
    return Q, (fx, fy, qx + K_OFFSET[0], qy + K_OFFSET[1])


def direct_mutants(Q, K4, w, h):
    """[(name, Q', K4')]: the four camera mutants, Q[3][3] read from a zero cell, the principal point taken from Q"""
    out = [(n, Q, k) for n, k in mutants(K4, w, h)]
    Q0 = np.array(Q, np.float64)
    Q0[3, 3] = 0.0
    out.append(("Q33:=0", Q0, K4))
    out.append(("c:=Q's", Q, (K4[0], K4[1], -Q[0, 3], -Q[1, 3])))
    return out


def full_Q(w, h):
    """a Q with all 16 entries non-zero: the standard five-entry form plus 1e-3-sized entries everywhere else (Q[3][0], Q[3][1] among
    them), no two of them equal"""
    Q, _ = direct_rig(w, h)
    fill = 1e-3 * (1.0 + np.arange(16).reshape(4, 4) / 7.0) * np.where((np.arange(16).reshape(4, 4) % 3) == 0, -1.0, 1.0)
    Q = np.where(Q != 0, Q, fill)
    Q[0, 0], Q[1, 1] = 1.0, 1.0
    return Q


def q_mutants(Q):
    """[(name, Q')]: each of the 16 entries read as zero (a kernel that ignores the entry, or reads it from a zero cell), and Q transposed"""
    out = []
    for i in range(4):
        for j in range(4):
            Qm = np.array(Q, np.float64)
            Qm[i, j] = 0.0
            out.append(("Q%d%d:=0" % (i, j), Qm))
    return out + [("Q^T", np.array(Q, np.float64).T.copy())]


REPROJECT_SHAPES = ((80, 60), (33, 17), (19, 16))       # (w, h): a planted field is at least 16 x 16


def disparity(w, h):
    """float32 disparities on the 1 / 16 grid, -2 .. 20, with zeros and negative values (no value makes Q[3] . v vanish: 4 d + 0.8
    has no root on the grid)"""
    rng = np.random.default_rng([3, w, h])
    d = (rng.integers(-32, 321, (h, w)) / 16.0).astype(np.float32)
    d[rng.random((h, w)) < 0.1] = 0.0
    d[0, 0], d[h - 1, w - 1] = 0.0, -1.0
    return d


# ---- the monocular pose tail -------------------------------------------------------------------------------------------------------
# counts4 of the vote scenes: every candidate voted on in every scene, one scene per winner and one four-way tie
MONO_VOTES = {"winner0": (9, 3, 2, 1), "winner1": (3, 9, 2, 1), "winner2": (2, 1, 9, 3), "winner3": (1, 2, 3, 9), "tie": (5, 5, 5, 5)}


def mono_scenes(K4=K_640):
    """{name: dict(E, p1, p2[, q, t, na, nb, depth_a, gate, mask])} built with planted_mono's builders under K4"""
    import planted_mono as PM
    E = PM.essential(1)
    out = {}
    for k, (name, counts4) in enumerate(MONO_VOTES.items()):
        p1, p2 = PM.plant_votes(E, counts4, np.random.default_rng([83, k]), K4=K4)
        out[name] = dict(E=E, p1=p1, p2=p2, depth_a=np.full(len(p1), 3.0), counts4=counts4)
    # the parallax gate: 24 inliers with sin2 from GATE / 4 to 4 GATE, the gate between them
    R, t = PM.pose(3, tdir=(1.0, 0.1, 0.2), angle=0.1)
    fac = np.exp(np.linspace(np.log(0.25), np.log(4.0), 24))
    p1, p2 = PM.plant_parallax(R, t, [PM.GATE * f for f in fac], K4=K4)
    out["gate"] = dict(E=PM.skew(t) @ R, p1=p1, p2=p2, depth_a=np.full(24, 2.0), gate=PM.GATE, sin2=PM.sin2_of(R, t, p1, p2, K4))
    # shared depths behind indices: 65 correspondences among 70 | 300 keypoints, one in ten without a depth
    n, na, nb = 65, 70, 300
    p1, p2 = PM.plant_votes(E, (50, 5, 5, 5), np.random.default_rng(84), K4=K4)
    rng = np.random.default_rng(85)
    q, t_ = rng.permutation(na)[:n].astype(np.int32), rng.permutation(nb)[:n].astype(np.int32)
    depth_a = np.where(rng.random(na) < 0.1, 0.0, rng.uniform(1.0, 5.0, na))
    out["shared_depth"] = dict(E=E, p1=p1, p2=p2, q=q, t=t_, na=na, nb=nb, depth_a=depth_a)
    # one size across the 1024-thread stride
    n = 1025
    k = n // 8
    p1, p2 = PM.plant_votes(E, (n - 3 * k, k, k, k), np.random.default_rng(86), K4=K4)
    rng = np.random.default_rng(87)
    out["n1025"] = dict(E=E, p1=p1, p2=p2, depth_a=np.where(rng.random(n) < 0.1, 0.0, rng.uniform(1.0, 9.0, n)), counts4=(n - 3 * k, k, k, k))
    return out


def mono_args(s, K4):
    """the arguments of recover_pose (device and restatement alike) of a scene"""
    return (s["E"], s["p1"], s["p2"], list(K4), s.get("mask"), s.get("q"), s.get("t"), s.get("na"), s.get("nb"), s.get("depth_a"), s.get("gate", 0.0))


MONO_PAIR_ARGS = (256, 1.0, 4321)          # iters, thr, seed of the fused finish's case: planted_mono's "eight" frames, solver 8


# ---- the PnP step ------------------------------------------------------------------------------------------------------------------
def pnp_cases():
    """{name: PnpCase under K_640}: M = 65 and M = 300 with 0.3 px noise and three refit steps, one through the windowed matcher, and
    the LO case (run with LO_RUN rounds x steps)"""
    from planted_pnp import PnpCase

    class GenericPnpCase(PnpCase):
        K4 = K_640

    return dict(M65=GenericPnpCase("generic_M65", 68, 65, n_in=45, noise=0.3, refine=3),
                M300=GenericPnpCase("generic_M300", 303, 300, n_in=200, noise=0.3, refine=3),
                window=GenericPnpCase("generic_window_M300", 303, 300, n_in=200, noise=0.3, refine=3, window=(80, 60)),
                lo=GenericPnpCase("generic_lo_n257", 260, 257, n_in=180, noise=1.0, refine=3))


LO_RUN = (2, 3)                            # rounds, steps


def with_camera(case, K4):
    """a copy of a built PnpCase whose MODEL scores under another camera (the planted inputs stay the generic camera's)"""
    import copy
    case.build()
    c = copy.copy(case)
    c.K4, c._model = tuple(K4), None
    c.__dict__.pop("_lo", None)
    return c


# ---- the Lucas-Kanade PnP step -----------------------------------------------------------------------------------------------------
KLT_W, KLT_H = 160, 120
K_KLT = generic(KLT_W, KLT_H)              # (144.0, 126.72, 75.5, 65.8)
KLT_CASE = dict(name="generic_sparse_refine3_n65", n=65, dense=False, refine=3, K4=K_KLT)


# ---- the landmark map --------------------------------------------------------------------------------------------------------------
MAP_KINDS = ("inside", "left_in", "left_out", "right_in", "right_out", "top_in", "top_out", "bottom_in", "bottom_out", "near_in", "near_out", "behind")


def map_scene(pose_cw, K4, z_min, org, crop, n_inside=120, per_kind=7, seed=0):
    """-> (scene dict as the map suites plant it, kind per landmark): landmarks that project inside the window, within 6 px inside and
    outside each of its four edges, just beyond and just before z_min, and behind the camera -- under pose_cw and K4"""
    rng = np.random.default_rng([91, seed])
    fx, fy, cx, cy = K4
    cw, ch = crop

    def cam(u, v, z):
        u, v, z = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(z, np.float64))
        return np.stack([(u + org[0] - cx) / fx * z, (v + org[1] - cy) / fy * z, z], -1)

    m = per_kind
    U, V, Zs = (lambda: rng.uniform(20, cw - 20, m)), (lambda: rng.uniform(20, ch - 20, m)), (lambda: rng.uniform(1.0, 12.0, m))
    near, far = rng.uniform(1.0, 6.0, m), rng.uniform(1.0, 6.0, m)
    parts = [("inside", cam(rng.uniform(8, cw - 9, n_inside), rng.uniform(8, ch - 9, n_inside), rng.uniform(1.0, 12.0, n_inside))),
             ("left_in", cam(near, V(), Zs())), ("left_out", cam(-far, V(), Zs())),
             ("right_in", cam(cw - 1 - near, V(), Zs())), ("right_out", cam(cw - 1 + far, V(), Zs())),
             ("top_in", cam(U(), near, Zs())), ("top_out", cam(U(), -far, Zs())),
             ("bottom_in", cam(U(), ch - 1 - near, Zs())), ("bottom_out", cam(U(), ch - 1 + far, Zs())),
             ("near_in", cam(U(), V(), z_min * rng.uniform(1.05, 1.5, m))), ("near_out", cam(U(), V(), z_min * rng.uniform(0.5, 0.95, m))),
             ("behind", cam(U(), V(), -rng.uniform(0.5, 9.0, m)))]
    Xc = np.concatenate([p for _, p in parts])
    kind = np.concatenate([np.full(len(p), MAP_KINDS.index(k)) for k, p in parts])
    order = rng.permutation(len(Xc))
    Xc, kind = Xc[order], kind[order]
    Rt = np.asarray(pose_cw, np.float64)
    xyz = ((Xc - Rt[:, 3]) @ Rt[:, :3]).astype(np.float32)
    n = len(xyz)
    scene = dict(xyz=xyz, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), rdesc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                 octave=rng.integers(0, 8, n).astype(np.int32), obs=rng.integers(1, 8, n).astype(np.int32), last=rng.integers(15, 20, n).astype(np.int32),
                 capacity=n + 200)
    return scene, kind


def map_frame(view, K4, org, crop, motion, rng, M_want=100, extra=7, noise=0.3, at_projection=0.7):
    """the frame a view is matched against, as the map suites build it but under K4: M of the view's keypoints seen again (descriptors
    with up to two bits flipped) from a camera moved by motion = (R, t), seven in ten at their projection (+ noise)"""
    import planted as P
    fx, fy, cx, cy = K4
    V = len(view["xy"])
    Mw = min(V, M_want)
    nt = Mw + extra
    desc = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q, t = np.sort(rng.choice(V, Mw, replace=False)), rng.permutation(nt)[:Mw]
    R, tv = motion
    xy = np.stack([rng.uniform(0, crop[0], nt), rng.uniform(0, crop[1], nt)], 1)
    xyz = P._cloud(nt, rng)
    for k in range(Mw):
        desc[t[k]] = view["desc"][q[k]]
        for bit in rng.choice(256, int(rng.integers(0, 3)), replace=False):
            desc[t[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
        Y = R @ view["xyz"][q[k]].astype(np.float64) + tv
        xyz[t[k]] = Y + rng.normal(0, 1e-3, 3)
        if rng.random() < at_projection:
            xy[t[k]] = [fx * Y[0] / Y[2] + cx - org[0] + noise * rng.normal(), fy * Y[1] / Y[2] + cy - org[1] + noise * rng.normal()]
    return dict(xy=xy.astype(np.float32), desc=desc, xyz=xyz.astype(np.float32), rdesc=rng.integers(0, 256, (nt, 32), dtype=np.uint8),
                octave=np.zeros(nt, np.int32), q=q, t=t)
