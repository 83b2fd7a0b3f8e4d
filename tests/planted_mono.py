"""Inputs for the planted tests of the monocular pose tail (vo_recover_pose: rp_tail and rs_svd3 in csrc/ransac.hip).  No GPU in
here: numpy and tests/mono_pose_ref.py (the restatement) only.

The tail decides by signs and comparisons, so a scene is PLANTED to force the decision, with a margin that keeps the device's
float64 on the same side of every sign test, and the builder re-checks what it planted with the restatement:

    candidates(E)                 the four (R, t) in the kernel's order: plus_1, minus_1, plus_2, minus_2
    plant_votes(E, counts4, rng)  float32 pixel pairs: counts4[c] points in front of both cameras under candidate c -- a pair on
                                  the epipolar geometry votes for exactly one candidate, so the votes ARE counts4
    plant_no_vote(E, m, rng)      off-epipolar pairs with mixed signs under both rotations: they vote for none of the four
    plant_parallax(R, t, ...)     pairs whose sin2 sits a chosen relative distance (down to 1e-10) above or below a target
    essentials()                  named 3x3 matrices for every arm of rs_svd3: true essentials, rank 1, a w2 / w0 ladder across the
                                  1e-14 repair threshold, scaled, column orders for the three-compare sort, zero, NaN, Inf
    SELECT_CASES / select_depths  depth_a for the radix select of the lower median, from the device's own z1
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mono_pose_ref as ref                # noqa: E402

K4 = (400.0, 400.0, 320.0, 240.0)
Z_MARGIN = 1e-3                            # min(|z1|, |z2|) of every planted pair under either rotation
PIX_MAX = 4000.0                           # |pixel| of every planted point


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = float(np.linalg.norm(r))
    if th == 0.0:
        return np.eye(3)
    k = skew(r / th)
    return np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)


def pose(seed, tdir=None, angle=0.25):
    """a rotation of `angle` rad about a random axis and a unit translation (random, or along tdir)"""
    rng = np.random.default_rng([77, seed])
    ax = rng.normal(size=3)
    t = rng.normal(size=3) if tdir is None else np.asarray(tdir, np.float64)
    return rodrigues(ax / np.linalg.norm(ax) * angle), t / np.linalg.norm(t)


def essential(seed, sign=1.0, **kw):
    R, t = pose(seed, **kw)
    return sign * (skew(t) @ R)


def candidates(E):
    R1, R2, t = ref.decompose(E)
    return [(R1, t), (R1, -t), (R2, t), (R2, -t)]


def traces(E):
    R1, R2, _ = ref.decompose(E)
    return (float(R1[0, 0]) + float(R1[1, 1])) + float(R1[2, 2]), (float(R2[0, 0]) + float(R2[1, 1])) + float(R2[2, 2])


def pixels(x, K4=K4):
    """normalised float64 points -> float32 pixels"""
    x = np.asarray(x, np.float64).reshape(-1, 2)
    return np.stack([x[:, 0] * K4[0] + K4[2], x[:, 1] * K4[1] + K4[3]], 1).astype(np.float32)


def classes(E, p1, p2, K4=K4):
    """per pair: the candidate 0 .. 3 it votes for (-1: none), and whether it keeps Z_MARGIN from every sign test"""
    R1, R2, t = ref.decompose(E)
    x1, x2 = ref.normalise(p1, K4), ref.normalise(p2, K4)
    cls = np.full(len(x1), -1)
    n_votes = np.zeros(len(x1), int)
    safe = np.ones(len(x1), bool)
    for k, R in enumerate((R1, R2)):
        z1, z2, _ = ref.depths(R, t, x1, x2)
        with np.errstate(invalid="ignore"):
            safe &= np.minimum(np.abs(z1), np.abs(z2)) >= Z_MARGIN
            plus, minus = (z1 > 0) & (z2 > 0), (z1 < 0) & (z2 < 0)
        cls[plus], cls[minus] = 2 * k, 2 * k + 1
        n_votes += plus.astype(int) + minus
    cls[n_votes != 1] = np.where(n_votes[n_votes != 1] == 0, -1, -2)      # (-2: more than one vote -- never planted)
    return cls, safe


def plant_votes(E, counts4, rng, K4=K4, shuffle=True):
    """float32 pixel pairs (p1, p2): counts4[c] of them triangulate in front of both cameras under candidate c."""
    cands = candidates(E)
    P1, P2 = [], []
    for c, (R, t) in enumerate(cands):
        need, rounds = int(counts4[c]), 0
        while need > 0:
            rounds += 1
            if rounds > 200:
                raise RuntimeError("candidate %d: no points in front of both cameras within the pixel range" % c)
            m = max(256, 3 * need)
            Z = np.exp(rng.uniform(np.log(0.5), np.log(20.0), m))
            xy = rng.uniform(-1.5, 1.5, (m, 2))
            Y = np.c_[xy * Z[:, None], Z] @ R.T + t
            ok = Y[:, 2] > 0.05
            with np.errstate(all="ignore"):
                p1, p2 = pixels(xy, K4), pixels(Y[:, :2] / Y[:, 2:], K4)
            ok &= np.isfinite(p2).all(1) & (np.abs(p2).max(1) <= PIX_MAX)
            p2[~ok] = 0.0
            cls, safe = classes(E, p1, p2, K4)
            ok &= safe & (cls == c)
            take = np.flatnonzero(ok)[:need]
            P1.append(p1[take])
            P2.append(p2[take])
            need -= len(take)
    n = int(np.sum(counts4))
    p1 = np.concatenate(P1) if n else np.zeros((0, 2), np.float32)
    p2 = np.concatenate(P2) if n else np.zeros((0, 2), np.float32)
    if shuffle:
        order = rng.permutation(n)
        p1, p2 = p1[order], p2[order]
    # what was planted is what the restatement counts
    R1, R2, t = ref.decompose(E)
    votes4, _ = ref.vote(R1, R2, t, ref.normalise(p1, K4), ref.normalise(p2, K4), np.ones(n, bool))
    assert list(votes4) == [int(c) for c in counts4], (votes4, counts4)
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2)


def plant_no_vote(E, m, rng, K4=K4):
    """m float32 pixel pairs off the epipolar geometry whose depths have mixed signs under BOTH rotations: votes4 = 0, 0, 0, 0."""
    P1, P2, need, rounds = [], [], m, 0
    while need > 0:
        rounds += 1
        if rounds > 200:
            raise RuntimeError("no pair without a vote found")
        k = max(256, 8 * need)
        p1 = rng.uniform([0, 0], [640, 480], (k, 2)).astype(np.float32)
        p2 = rng.uniform([0, 0], [640, 480], (k, 2)).astype(np.float32)
        cls, safe = classes(E, p1, p2, K4)
        take = np.flatnonzero(safe & (cls == -1))[:need]
        P1.append(p1[take])
        P2.append(p2[take])
        need -= len(take)
    p1, p2 = np.concatenate(P1), np.concatenate(P2)
    R1, R2, t = ref.decompose(E)
    votes4, _ = ref.vote(R1, R2, t, ref.normalise(p1, K4), ref.normalise(p2, K4), np.ones(m, bool))
    assert not votes4.any()
    return p1, p2


def sin2_of(R, t, p1, p2, K4=K4):
    return ref.depths(R, t, ref.normalise(p1, K4), ref.normalise(p2, K4))[2]


U0_PIX = 0.002        # x pixel of the second view of every parallax pair: a float32 that small resolves 2.3e-10 pixels


def plant_parallax(R, t, sin2_targets, rel_offsets=None, seed=0, K4=K4):
    """One float32 pixel pair per target whose sin2 -- as the restatement computes it under (R, t) -- is
    target * (1 + rel_offset) to within 1e-10 relative: rel_offset > 0 above the target, < 0 below, |rel_offset| down to 2e-10.

    Float32 pixels of a few hundred resolve sin2 to 1e-5 relative only.  So the second view's x pixel is put next to 0 (U0_PIX),
    where float32 resolves 2.3e-10 pixels; the depth is bisected until sin2 meets the target, the first view is rounded to
    float32, and that x pixel alone is then bisected in float64 and rounded.  t must have an x component for x to move sin2."""
    rng = np.random.default_rng([5, seed])
    fx, fy, cx, cy = K4
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    if rel_offsets is None:
        rel_offsets = np.zeros(len(sin2_targets))
    P1, P2 = [], []

    def s2(p1, u, v):
        return float(ref.depths(R, t, ref.normalise(p1, K4), np.array([[(u - cx) / fx, (v - cy) / fy]]))[2][0])

    for target, off in zip(sin2_targets, rel_offsets):
        want = float(target) * (1.0 + float(off))
        for _ in range(50):
            v = float(np.float32(rng.uniform(40.0, 440.0)))
            h2 = np.array([(U0_PIX - cx) / fx, (v - cy) / fy, 1.0])

            def first_view(z2):
                X = R.T @ (z2 * h2 - t)
                return X, pixels(X[None, :2] / X[2], K4)
            lo, hi = 0.3, 1e5                                  # sin2 falls as the point recedes
            if not (s2(first_view(lo)[1], U0_PIX, v) > want > s2(first_view(hi)[1], U0_PIX, v)):
                continue
            for _ in range(60):
                mid = np.sqrt(lo * hi)
                lo, hi = (mid, hi) if s2(first_view(mid)[1], U0_PIX, v) > want else (lo, mid)
            X, p1 = first_view(lo)
            if X[2] < 0.05 or np.abs(p1).max() > PIX_MAX:
                continue
            # p1 is float32 now: move the x pixel of the second view alone
            a, b = U0_PIX - 0.0015, U0_PIX + 0.0015
            fa, fb = s2(p1, a, v) - want, s2(p1, b, v) - want
            if not fa * fb < 0:
                continue
            for _ in range(60):
                mid = 0.5 * (a + b)
                fm = s2(p1, mid, v) - want
                a, b, fa = (mid, b, fm) if fa * fm > 0 else (a, mid, fa)
            p2 = np.array([[np.float32(0.5 * (a + b)), np.float32(v)]], np.float32)
            got = float(sin2_of(R, t, p1, p2, K4)[0])
            if abs(got / want - 1.0) <= 1e-10:
                P1.append(p1[0])
                P2.append(p2[0])
                break
        else:
            raise RuntimeError("no pair with sin2 = %g found" % want)
    return np.array(P1, np.float32), np.array(P2, np.float32)


# ---- essential matrices for every arm of rs_svd3 ----------------------------------------------------------------------------
def _orth(seed):
    """a random rotation (det +1)"""
    Q, _ = np.linalg.qr(np.random.default_rng([11, seed]).normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


LADDER = (0.0, 1e-15, 1e-14, 2e-14, 1e-12, 1e-8)
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def essentials():
    """[(name, E, kind)]; kind: "full" (w1 > 0: t is LAPACK's third left singular vector), "rank1" (only orthonormality and
    t perpendicular to u0 are defined) or "refused" (zero / non-finite: flags bit 0)."""
    out = []
    R, t = pose(3, tdir=(0.3, -0.2, 1.0))
    out += [("skew+", skew(t) @ R, "full"), ("skew-", -(skew(t) @ R), "full")]
    # rank 1: u v^T with v an axis, so that two columns are exactly zero and w1 = 0 exactly (a general v leaves w1 ~ 1e-17 w0)
    ux, uy = np.array([0.96, 0.2, -0.1]), np.array([0.3, -0.5, 0.8])
    out += [("rank1_x", np.outer(ux, [1.0, 0.0, 0.0]), "rank1"), ("rank1_y", np.outer(uy, [0.0, 0.0, 1.0]), "rank1")]
    U, V = _orth(1), _orth(2)
    out.append(("fullrank_1e-3", U @ np.diag([1.0, 0.8, 1e-3]) @ V.T, "full"))
    for rel in LADDER:
        out.append(("ladder_%g" % rel, U @ np.diag([1.0, 1.0, rel]) @ V.T, "full"))
    out += [("scaled_1e-6", 1e-6 * (skew(t) @ R), "full"), ("scaled_1e6", 1e6 * (skew(t) @ R), "full")]
    # E = U diag(w) with w permuted: the columns are orthogonal already, no sweep reorders them, and the largest singular value
    # stays in the column it was put in -- every outcome of the three-compare sort
    w = np.array([1.0, 0.9, 0.0])
    for perm in PERMS:
        out.append(("order_%d%d%d" % perm, _orth(4) * w[list(perm)][None, :], "full"))
    nan, inf = skew(t) @ R, skew(t) @ R
    nan[1, 2], inf[2, 0] = np.nan, np.inf
    out += [("zero", np.zeros((3, 3)), "refused"), ("nan", nan, "refused"), ("inf", inf, "refused")]
    return out


# ---- the select ---------------------------------------------------------------------------------------------------------------
SELECT_N = 1024
NO_DEPTH = (0.0, -1.0, np.inf, np.nan)     # values of depth_a that do not count
SELECT_CASES = ("all_equal", "split_511_513", "split_512_512", "low_bytes", "top_bytes", "run_300", "extremes",
                "shared_1", "shared_2", "shared_3", "shared_255", "shared_256", "shared_257")
LOW_BYTES_START = 0x3FEFFFFFFFFFFE00


def select_targets(case, n=SELECT_N):
    """-> (target ratios r, shared) for n correspondences; shared[i] False: depth_a gets a value from NO_DEPTH."""
    rng = np.random.default_rng([9, SELECT_CASES.index(case)])
    shared = np.ones(n, bool)
    if case == "all_equal":
        r = np.full(n, 2.0)
    elif case.startswith("split"):
        lo = int(case.split("_")[1])
        r = np.where(np.arange(n) < lo, 0.5, 2.0)              # top bytes 0x3F | 0x40: rank 511 on the edge of a scan lane's four bins
    elif case == "low_bytes":
        r = (np.uint64(LOW_BYTES_START) + np.arange(n, dtype=np.uint64)).view(np.float64)
    elif case == "top_bytes":
        r = 2.0 ** np.round(np.linspace(-400, 400, n))
    elif case == "run_300":
        r = np.concatenate([rng.uniform(0.2, 0.99, 362), np.full(300, 1.0), rng.uniform(1.01, 5.0, n - 662)])   # ranks 362 .. 661 equal
    elif case == "extremes":
        r = np.concatenate([np.full(400, 0.0), rng.uniform(0.5, 2.0, 111), np.full(n - 511, np.inf)])
    else:
        k = int(case.split("_")[1])
        r = rng.uniform(0.5, 2.0, n)
        shared[:] = False
        shared[rng.permutation(n)[:k]] = True
    order = rng.permutation(n)
    return r[order], shared[order]


def select_depths(case, z1):
    """depth_a (identity indices) for a select case from the z1 the device returned.  Power-of-two ratios are met exactly
    (d = r z1 and d / z1 are exact); the others to an ulp: the test's reference is the median of the ACTUAL d / z1.
    "extremes": ratios that underflow to 0 and overflow to inf (both are values; neither is the ~0 pattern of "none")."""
    z1 = np.asarray(z1, np.float64)
    r, shared = select_targets(case, len(z1))
    with np.errstate(over="ignore"):
        d = r * z1
    if case == "extremes":
        d = np.where(r == 0.0, 5e-324, np.where(np.isinf(r), 1.7e308, d))
    none = np.flatnonzero(~shared)
    d[none] = np.asarray(NO_DEPTH)[np.arange(len(none)) % len(NO_DEPTH)]
    return d, shared


def actual_ratios(d, z1, valid=None):
    """the ratios the device must select among, in numpy: depth_a / z1 over the valid pairs with a positive finite depth"""
    d, z1 = np.asarray(d, np.float64), np.asarray(z1, np.float64)
    with np.errstate(all="ignore"):
        sh = (d > 0) & np.isfinite(d)
        if valid is not None:
            sh &= valid
        return (d / z1)[sh], sh


# ---- the cases of tests/test_gpu_planted_mono.py (tests/test_planted_mono_ref.py checks them on the CPU) -------------------------
VOTE_COUNTS = ((5, 5, 0, 0), (0, 0, 5, 5), (5, 0, 5, 0), (0, 5, 0, 5), (5, 0, 0, 5), (0, 5, 5, 0), (3, 3, 3, 3), (4, 5, 5, 5), (1, 0, 0, 0),
               (0, 0, 0, 1), (0, 0, 0, 0))
ALL_TIE_ARMS = {("same", 0), ("same", 1), ("v2", True), ("v2", False), ("v3", True), ("v3", False)}


def vote_essentials():
    """both signs of one E (tr R1 > tr R2 and the reverse) and another with tr R1 < tr R2"""
    return [("A+", essential(1)), ("A-", essential(1, -1.0)), ("B", essential(5))]


def vote_scene(E, counts4, seed):
    rng = np.random.default_rng([21, seed])
    if any(counts4):
        return plant_votes(E, counts4, rng)
    return plant_no_vote(E, 12, rng)


def tie_arms(v, tr1, tr2):
    """the ties met on the way to the winner, each with the way it went: ("v2" | "v3", whether the trace moved the winner) for a
    tie between the rotations, ("same", pair) for a tie inside rotation `pair`, where the trace cannot decide"""
    arms, best, bv, bt = set(), 0, v[0], tr1
    if v[1] == bv:
        arms.add(("same", 0))
    if v[1] > bv:
        best, bv = 1, v[1]
    if v[2] == bv:
        arms.add(("v2", tr2 > bt))
    if v[2] > bv or (v[2] == bv and tr2 > bt):
        best, bv, bt = 2, v[2], tr2
    if v[3] == bv:
        arms.add(("same", 1) if best == 2 else ("v3", tr2 > bt))
    return arms


GATE = float(np.sin(np.deg2rad(0.5)) ** 2)
GATE_NEAR = (2e-10, 4e-10, 6e-10, 8e-10, -2e-10, -4e-10, -6e-10, -8e-10)
_gate_scene = []


def gate_scene():
    """one pose, 64 inliers: 56 with sin2 from GATE / 4 to 4 GATE (none within 1 % of it), then four within 1e-9 relative above
    GATE and four as close below (1e-11 at the least: the device's 1e-12 cannot move them across)"""
    if not _gate_scene:
        R, t = pose(3, tdir=(1.0, 0.1, 0.2), angle=0.1)
        fac = np.exp(np.linspace(np.log(0.25), np.log(4.0), 56))
        assert (np.abs(fac - 1.0) > 0.01).all()
        p1, p2 = plant_parallax(R, t, [GATE * f for f in fac] + [GATE] * 8, [0.0] * 56 + list(GATE_NEAR))
        rel = sin2_of(R, t, p1, p2)[56:] / GATE - 1.0
        assert (rel[:4] > 1e-11).all() and (rel[:4] < 1e-9).all() and (rel[4:] < -1e-11).all() and (rel[4:] > -1e-9).all(), rel
        _gate_scene.append(dict(E=skew(t) @ R, R=R, t=t, p1=p1, p2=p2))
    return _gate_scene[0]


STRIDE_SIZES = (1023, 1024, 1025, 2047, 2049, 65536)


def stride_scene(n):
    """n planted pairs with votes for all four candidates (the first by far the most)"""
    k = n // 8
    return plant_votes(essential(1), (n - 3 * k, k, k, k), np.random.default_rng([31, n]))


def last_of_word_mask(n):
    """inliers: only the last element of each 64-word"""
    return (np.arange(n) % 64 == 63).astype(np.uint8)


# ---- frames for the fused finish (k_mono_pose_finish) -------------------------------------------------------------------------
# seed -> the matches that survive ORB (2000 features) + kNN-2 + ratio 0.8 between the two frames, as the CPU oracle counts them
# (tests/test_planted_mono_ref.py): below the minimum of either solver, the 5-point solver's minimum, the 8-point solver's
FINISH_SEEDS = {"too_few": (22, 3), "six": (86, 6), "eight": (8, 8)}
FINISH_RATIO = 0.8


def finish_frames(seed):
    """two 640 x 480 frames: one small plain rectangle of low contrast on a flat background, and the same shifted by a few pixels"""
    rng = np.random.default_rng([17, seed])
    a = np.full((480, 640), 90, np.uint8)
    w, h = int(rng.integers(3, 14)), int(rng.integers(3, 14))
    x, y = int(rng.integers(100, 500)), int(rng.integers(100, 340))
    a[y:y + h, x:x + w] = 90 + int(rng.integers(22, 80))
    dx, dy = int(rng.integers(3, 9)), int(rng.integers(-4, 5))
    b = np.full_like(a, 90)
    b[max(dy, 0):480 + min(dy, 0), dx:] = a[max(-dy, 0):480 + min(-dy, 0), :640 - dx]
    return a, b
