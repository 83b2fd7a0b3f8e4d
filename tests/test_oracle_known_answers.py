"""Analytic known-answer tests pinning the oracle's restatement of the cv2 stages (the reference
holds no fixture for them -- SURVEY.md section 4)."""
import numpy as np

from openvo_amd.synth import Corridor

P = dict(minDisparity=0, numDisparities=32, blockSize=5, P1=200, P2=800, disp12MaxDiff=1, preFilterCap=63,
         uniquenessRatio=10, speckleWindowSize=100, speckleRange=2)


def _texture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2)).astype(np.float64)
    a = np.kron(a, np.ones((4, 4)))[:h, :w]
    a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, 2, 1)) / 4
    return a.astype(np.uint8)


def test_sgbm_constant_disparity_plane(oracle):
    L = _texture(96, 200, 1)
    d = 7
    R = np.roll(L, -d, axis=1)           # right image sees the scene shifted left by d
    for mode in (0, 1):
        disp = oracle.sgbm_compute(L, R, P, mode)
        assert disp.dtype == np.int16 and disp.shape == L.shape
        assert (disp[:, :32] == -16).all()                      # columns < numDisparities: INVALID = (minD-1)*16
        inner = disp[8:-8, 48:-16]
        assert (inner == d * 16).mean() > 0.97                  # exact integer disparity, zero sub-pixel offset


def test_sgbm_subpixel_and_float_conversion(oracle):
    c = Corridor("T0")
    L, R = c.pair(0)
    disp = oracle.sgbm_compute(L, R, c.sgbm_params(), 0)
    f = disp.astype(np.float32) / 16                            # reference stereo_camera.py:51, exact in f32
    assert np.array_equal((f * 16).astype(np.int16), disp)
    # ground plane row v: d = B (v - cy) / 1.65
    v = 200
    row = f[v][(f[v] > 0)]
    assert abs(np.median(row) - c.B * (v - c.cy) / 1.65) < 0.25


def test_cost_volume_definition(oracle):
    """C = P2 + 5x5 replicate-border box sum of the BT pixel cost; checked by brute force."""
    rng = np.random.default_rng(3)
    L = rng.integers(0, 256, (12, 48), dtype=np.uint8)
    R = rng.integers(0, 256, (12, 48), dtype=np.uint8)
    p = dict(P, numDisparities=16)
    C = oracle.sgbm_cost_volume(L, R, p).astype(np.int64)
    h, w = L.shape
    D, ft = 16, 63

    def chan(img, c):
        I = img.astype(np.int64)
        if c == 1:
            out = I.copy()
        else:
            Ip = np.pad(I, ((1, 1), (0, 0)), mode="edge")
            out = np.zeros_like(I)
            for y in range(h):
                for x in range(1, w - 1):
                    g = (Ip[y + 1, x + 1] - Ip[y + 1, x - 1]) * 2 + Ip[y, x + 1] - Ip[y, x - 1] + Ip[y + 2, x + 1] - Ip[y + 2, x - 1]
                    out[y, x] = min(max(g, -ft), ft) + ft
        out[:, 0] = out[:, -1] = ft
        return out

    def bounds(a):
        lo, hi = a.copy(), a.copy()
        for x in range(w):
            vl = (a[:, x] + a[:, x - 1]) // 2 if x > 0 else a[:, x]
            vr = (a[:, x] + a[:, x + 1]) // 2 if x < w - 1 else a[:, x]
            lo[:, x] = np.minimum(np.minimum(vl, vr), a[:, x])
            hi[:, x] = np.maximum(np.maximum(vl, vr), a[:, x])
        return lo, hi

    W1 = w - D
    pix = np.zeros((h, W1, D), np.int64)
    for c in (0, 1):
        u, v = chan(L, c), chan(R, c)
        u0, u1 = bounds(u)
        v0, v1 = bounds(v)
        for x1 in range(W1):
            x = x1 + D
            for d in range(D):
                c0 = np.maximum(np.maximum(0, u[:, x] - v1[:, x - d]), v0[:, x - d] - u[:, x])
                c1 = np.maximum(np.maximum(0, v[:, x - d] - u1[:, x]), u0[:, x] - v[:, x - d])
                pix[:, x1, d] += np.minimum(c0, c1) >> (0 if c == 0 else 2)
    pp = np.pad(pix, ((2, 2), (2, 2), (0, 0)), mode="edge")
    box = sum(pp[2 + j: 2 + j + h, 2 + i: 2 + i + W1] for j in range(-2, 3) for i in range(-2, 3))
    assert np.array_equal(C, box + 800)


def test_median_and_speckle(oracle):
    rng = np.random.default_rng(4)
    img = rng.integers(-16, 2000, (20, 30)).astype(np.int16)
    med = oracle.median3x3_s16(img)
    p = np.pad(img, 1, mode="edge")
    ref = np.median(np.stack([p[1 + j: 21 + j, 1 + i: 31 + i] for j in (-1, 0, 1) for i in (-1, 0, 1)]), 0)
    assert np.array_equal(med, ref.astype(np.int16))
    d = np.full((20, 30), 320, np.int16)
    d[5:8, 5:8] = 800          # 9-pixel blob: removed when window >= 9
    d[12, 20] = -16            # already invalid
    assert (oracle.filter_speckles(d, -16, 9, 32)[5:8, 5:8] == -16).all()
    assert (oracle.filter_speckles(d, -16, 8, 32)[5:8, 5:8] == 800).all()
    out = oracle.filter_speckles(d, -16, 9, 32)
    assert (out[d == 320] == 320).all()


def test_sgbm_every_sum_saturated_in_the_last_column(oracle):
    """The saturating scene of tests/sgbm_def_cases.py in MODE_HH, at minDisparity 0 and -16: pixels whose eight path costs sum
    to 32767 and more at every disparity have no winner and come out invalid, the others (ratio 0, no left-right limit) valid.
    In the band's last column stereosgbm.cpp's bestDisp = -1 reads disp2cost[w], one element past the buffer; the oracle leaves
    that step out, and under the sanitizer build this test is the one that walks over the place.  At minDisparity -16 every row
    has such a pixel; at 0 the last column is ftzero against ftzero at d = 0 and one row has."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import sgbm_def
    import sgbm_def_cases as C
    for name, last in (("saturating-m1", 1), ("saturating-minD-16-m1", 24)):
        c = C.BY_NAME[name]
        assert c.p["minDisparity"] <= 0 and c.mode == 1
        e = sgbm_def.effective(c.p, c.w)
        L, R = C.images(c)
        d, info = C.definition(c)
        none = (d["S"] == sgbm_def.MAX_S).all(axis=2)
        assert none[:, -1].sum() >= last and 100 <= none.sum() == info["no_winner"] <= none.size - 100
        raw, _, fin = oracle.sgbm_compute(L, R, c.p, 1, stages=True)
        band = raw[:, e.x0:e.x1]
        assert (band[none] == e.invalid).all() and (band[~none] >= e.minD * 16).all()
        assert np.array_equal(raw, d["raw"]) and np.array_equal(fin, d["final"])


def test_fast_corner_and_nms(oracle):
    img = np.full((40, 40), 50, np.uint8)
    img[20, 20] = 200                      # isolated bright pixel: all 16 ring pixels darker
    img[10, 30] = 90                       # contrast 40: corner with a lower score
    sm = oracle.fast_score_map(img, 20)
    ys, xs = np.nonzero(sm)
    assert sorted(zip(ys.tolist(), xs.tolist())) == [(10, 30), (20, 20)]
    assert sm[20, 20] == 149 and sm[10, 30] == 39   # largest threshold keeping it a corner
    img[20, 21] = 200                      # two equal neighbours: strict NMS suppresses both
    assert oracle.fast_score_map(img, 20)[20, 20:22].sum() == 0
    flat = np.full((40, 40), 77, np.uint8)
    assert oracle.fast_score_map(flat, 20).sum() == 0


def test_orb_quotas_canonical_order_and_rotation(oracle):
    c = Corridor("C1")
    L, _ = c.pair(1)
    k = oracle.orb_detect_and_compute(L, None, 500)
    n = len(k["xy"])
    assert 400 <= n <= 520
    cnt = np.bincount(k["octave"], minlength=8)
    assert (cnt <= np.array([109, 90, 75, 63, 52, 44, 36, 31]) + 3).all()
    scale = (1.2 ** k["octave"]).astype(np.float32)
    x, y = k["xy"][:, 0] / scale, k["xy"][:, 1] / scale
    key = k["octave"] * 1e8 + np.rint(y) * 1e4 + np.rint(x)
    assert (np.diff(key) > 0).all()                              # canonical (octave, y, x) order
    assert (k["angle"] >= 0).all() and (k["angle"] < 360).all()
    assert np.allclose(k["size"], 31 * scale)
    # the image rotated by 180 degrees gives angles rotated by 180 degrees for matching corners
    k2 = oracle.orb_detect_and_compute(L[::-1, ::-1].copy(), None, 500)
    lv0 = k["octave"] == 0
    p0 = {(int(a), int(b)): ang for (a, b), ang in zip(k["xy"][lv0], k["angle"][lv0])}
    h, w = L.shape
    hits = 0
    for (a, b), ang in zip(k2["xy"][k2["octave"] == 0], k2["angle"][k2["octave"] == 0]):
        q = (w - 1 - int(a), h - 1 - int(b))
        if q in p0:
            dd = abs(((ang - p0[q]) % 360) - 180)
            assert dd < 1e-3
            hits += 1
    assert hits > 20


def test_orb_mask_excludes_keypoints(oracle):
    c = Corridor("C1")
    L, _ = c.pair(1)
    mask = np.zeros_like(L)
    mask[:, : L.shape[1] // 2] = 255
    k = oracle.orb_detect_and_compute(L, mask, 500)
    assert len(k["xy"]) > 50 and (k["xy"][:, 0] < L.shape[1] // 2 + 1).all()


def test_resize_linear_exact_constant_and_ramp(oracle):
    a = np.full((30, 40), 131, np.uint8)
    assert (oracle.resize_linear_exact(a, 33, 25) == 131).all()
    ramp = np.tile(np.arange(0, 240, 2, dtype=np.uint8), (10, 1))
    out = oracle.resize_linear_exact(ramp, 100, 8).astype(int)
    assert (np.diff(out[0]) >= 0).all() and abs(out[0][50] - (1.2 * 50.5 - 0.5) * 2) <= 1.5


def test_bf_knn2_ties_and_ratio(oracle):
    t = np.zeros((5, 32), np.uint8)
    t[1, 0] = 0b1          # distance 1
    t[2, 0] = 0b10         # distance 1 (tie with row 1 -> lower index first)
    t[3, 0] = 0b111
    t[4] = 255
    q = np.zeros((1, 32), np.uint8)
    idx, dist = oracle.bf_knn2_hamming(q, t)
    assert idx.tolist() == [[0, 1]] and dist.tolist() == [[0, 1]]
    idx, dist = oracle.bf_knn2_hamming(q, t[1:])
    assert idx.tolist() == [[0, 1]] and dist.tolist() == [[1, 1]]
    qo, to = oracle.ratio_filter(np.array([[3, 4], [1, 2]], np.int32), np.array([[8, 10], [7, 10]], np.int32), 0.8)
    assert qo.tolist() == [1] and to.tolist() == [1]            # 8 < 0.8*10 is False (strict), 7 < 8 True


def test_umeyama_exact_rigid_motion_and_reflection(oracle):
    rng = np.random.default_rng(9)
    src = rng.normal(size=(50, 3)).astype(np.float32) * 3
    ang = 0.2
    Rm = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    t = np.array([0.3, -0.2, 1.0])
    dst = (src.astype(np.float64) @ Rm.T + t).astype(np.float32)
    T, s = oracle.umeyama(src, dst)
    assert np.allclose(T[:, :3], Rm, atol=1e-6) and np.allclose(T[:, 3], t, atol=1e-5) and abs(s - 1) < 1e-6
    assert abs(np.linalg.det(T[:, :3]) - 1) < 1e-12
    # a mirrored cloud must still give a proper rotation (force_rotation=True)
    T2, _ = oracle.umeyama(src, dst * np.array([1, 1, -1], np.float32))
    assert abs(np.linalg.det(T2[:, :3]) - 1) < 1e-9
    r = oracle.rodrigues(T[:, :3])
    assert abs(np.linalg.norm(r) - ang) < 1e-6 and abs(r[2, 0] - ang) < 1e-6
    assert np.allclose(oracle.rodrigues(np.eye(3)), 0)
    U, w, Vt = oracle.svd3(rng.normal(size=(3, 3)))
    assert w[0] >= w[1] >= w[2] >= 0 and np.allclose(U @ U.T, np.eye(3), atol=1e-12)


def test_reproject_matches_definition(oracle):
    c = Corridor("T0")
    Q = c.Q()
    disp = np.array([[16.0, 0.0, -1.0, 5.5]], np.float32)
    with np.errstate(all="ignore"):
        out = oracle.reproject_to_3d(disp, Q)
    z0 = c.f * c.B / 16.0
    assert abs(out[0, 0, 2] - z0) < 1e-4
    assert np.isinf(out[0, 1, 2])                                # d = 0 -> W = 0 -> inf
    assert out[0, 2, 2] < 0                                      # invalid disparity -1 gives finite garbage
    pts, st = oracle.points3d_at(np.array([[256, 0, -16, 88]], np.int16), Q, (0, 0, 4, 1), np.array([[0.0, 0.0], [3.0, 0.0]], np.float32))
    assert st.tolist() == [0, 0] and np.array_equal(pts[0], out[0, 0]) and np.array_equal(pts[1], out[0, 3])


def test_bgr2gray_and_remap(oracle):
    bgr = np.zeros((1, 4, 3), np.uint8)
    bgr[0, 0] = (255, 255, 255)
    bgr[0, 1] = (255, 0, 0)
    bgr[0, 2] = (0, 255, 0)
    bgr[0, 3] = (0, 0, 255)
    assert oracle.bgr2gray(bgr).tolist() == [[255, 29, 150, 76]]
    src = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3
    m1 = np.zeros((8, 8, 2), np.int16)
    m1[..., 0], m1[..., 1] = np.meshgrid(np.arange(8), np.arange(8))
    m2 = np.zeros((8, 8), np.uint16)
    assert np.array_equal(oracle.remap_bilinear(src, m1, m2), src)            # identity map
    m2[:] = 16                                                               # fx = 16/32: halfway to x+1
    out = oracle.remap_bilinear(src, m1, m2)
    assert out[0, 0] == (int(src[0, 0]) + int(src[0, 1]) + 1) // 2
    assert out[0, 7] == (int(src[0, 7]) * 16384 + (1 << 14)) >> 15           # x+1 outside: border 0


def test_p3p_recovers_synthetic_poses(oracle):
    """The PnP loop has no reference counterpart; its restatement is pinned by geometry instead: for
    random poses and triangles the true pose is among the P3P candidates (float64, 1e-7)."""
    rng = np.random.default_rng(0)
    for trial in range(300):
        r = rng.normal(size=3) * 0.3
        th = np.linalg.norm(r)
        k = r / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = rng.normal(size=3) * 0.5
        X = rng.uniform(-2, 2, (3, 3)) + np.array([0, 0, 6.0])
        Xc = X @ R.T + t
        y = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
        sols = oracle.p3p(y, X)
        assert 1 <= len(sols) <= 4
        assert min(np.abs(Rs - R).max() + np.abs(ts - t).max() for Rs, ts in sols) < 1e-7
        for Rs, ts in sols:   # every candidate is a rotation that reproduces the three bearings
            assert np.allclose(Rs @ Rs.T, np.eye(3), atol=1e-8) and np.linalg.det(Rs) > 0
            Yc = X @ Rs.T + ts
            assert np.allclose(Yc / np.linalg.norm(Yc, axis=1, keepdims=True), y, atol=1e-7)


def test_ransac_pnp_oracle_finds_the_pose(oracle):
    rng = np.random.default_rng(3)
    n, f, cx, cy = 400, 700.0, 320.0, 240.0
    X = np.stack([rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), rng.uniform(4, 30, n)], 1)
    R = np.eye(3)
    t = np.array([0.1, 0.0, -0.25])
    Xc = X @ R.T + t
    uv = np.stack([f * Xc[:, 0] / Xc[:, 2] + cx, f * Xc[:, 1] / Xc[:, 2] + cy], 1)
    out = rng.choice(n, 120, replace=False)
    uv[out] += rng.uniform(-50, 50, (120, 2))
    r = oracle.ransac_pnp(X, uv, [f, f, cx, cy], iters=200, thr=1.0, seed=7)
    assert r["best_count"] >= 280 and r["counts"].max() == r["best_count"] and r["counts"][r["best_iter"]] == r["best_count"]
    assert np.abs(r["Rt"][:, :3] - R).max() < 1e-3 and np.abs(r["Rt"][:, 3] - t).max() < 1e-2
    assert r["mask"].sum() == r["best_count"]


# ---- five-point essential solver (the build's own definition; the mathematics is pinned here) -------------------
def _motion_scene(rng, planar=False, n=6):
    from openvo_amd import calib
    R = calib.rodrigues_vec_to_mat(rng.normal(scale=0.1, size=3))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)]
    if planar:
        X[:, 2] = 6 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    X2 = X @ R.T + t * 0.5
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:], E / np.linalg.norm(E)


def test_five_point_solutions_satisfy_every_constraint(oracle):
    """Each returned matrix is a genuine essential matrix through the five correspondences: epipolar residuals at
    rounding level, det E = 0 and 2 E E^T E - tr(E E^T) E = 0 to the accuracy of the root bisection."""
    rng = np.random.default_rng(7)
    dets, cubics = [], []
    for _ in range(100):
        x1, x2, _E = _motion_scene(rng)
        sols = oracle.essential_5pt(x1[:5], x2[:5])
        assert 1 <= len(sols) <= 10
        for S in sols:
            assert abs(np.linalg.norm(S) - 1) < 1e-12
            res = [np.r_[b, 1] @ S @ np.r_[a, 1] for a, b in zip(x1[:5], x2[:5])]
            assert np.abs(res).max() < 1e-10
            dets.append(abs(np.linalg.det(S)))
            cubics.append(np.abs(2 * S @ S.T @ S - np.trace(S @ S.T) * S).max())
    dets, cubics = np.array(dets), np.array(cubics)
    assert len(dets) >= 300                                              # about 4.9 real solutions per sample on average
    # the cubic constraints hold to the conditioning of each root: nearly always to 1e-9, never worse than 1e-4
    assert np.median(dets) < 1e-12 and np.mean(dets < 1e-9) > 0.9 and dets.max() < 1e-4
    assert np.median(cubics) < 1e-12 and np.mean(cubics < 1e-9) > 0.9 and cubics.max() < 1e-4


def test_five_point_contains_the_true_motion(oracle):
    """Exact synthetic motions: the true E (up to sign) is among the candidates -- general scenes and the planar scenes
    that defeat the eight-point algorithm.  The small shortfall is conditioning (near-double roots), not missed roots."""
    for planar, need6, need3 in ((False, 0.97, 0.985), (True, 0.88, 0.93)):
        rng = np.random.default_rng(1)
        errs = []
        for _ in range(400):
            x1, x2, E = _motion_scene(rng, planar)
            sols = oracle.essential_5pt(x1[:5], x2[:5])
            errs.append(min([min(np.abs(S - E).max(), np.abs(S + E).max()) for S in sols]) if sols else 9.0)
        errs = np.array(errs)
        assert np.mean(errs < 1e-6) >= need6 and np.mean(errs < 1e-3) >= need3, (planar, np.mean(errs < 1e-6), np.mean(errs < 1e-3))
        assert np.median(errs) < 1e-10


def test_five_point_root_finder_separates_close_roots(oracle):
    """Roots much closer than any fixed sampling grid are each found (isolation between derivative roots), roots
    outside [-1, 1] are not reported, and a polynomial without real roots reports none."""
    P = np.polynomial.polynomial
    for gap in (1e-3, 1e-5, 1e-7):
        want = np.array([-0.9, -0.3, 0.2, 0.2 + gap, 0.75])
        c = P.polyfromroots(np.r_[want, 1.7, -2.5, 1.2 + 0.4j, 1.2 - 0.4j, 3.0])
        got = oracle.poly10_roots_unit(np.real(c) / np.abs(c).max())
        assert len(got) == 5 and np.abs(got - want).max() < max(1e-9, 1e-4 * gap) and (np.diff(got) > 0).all()
    none = P.polyfromroots([1j, -1j, 2j, -2j, 0.5 + 1j, 0.5 - 1j, -0.4 + 0.1j, -0.4 - 0.1j, 3.0, -3.0])
    assert len(oracle.poly10_roots_unit(np.real(none))) == 0
    ten = np.linspace(-0.95, 0.95, 10)
    got = oracle.poly10_roots_unit(np.real(P.polyfromroots(ten)))
    assert len(got) == 10 and np.abs(got - ten).max() < 1e-9


def test_five_point_degenerate_input_returns_nothing_or_finite(oracle):
    z = np.zeros((5, 2))
    assert oracle.essential_5pt(z, z) == [] or all(np.isfinite(S).all() for S in oracle.essential_5pt(z, z))
    x = np.tile([[0.1, 0.2]], (5, 1))                                    # five copies of one correspondence
    for S in oracle.essential_5pt(x, x + 0.01):
        assert np.isfinite(S).all()


def test_ransac_five_point_recovers_motion_with_outliers(oracle):
    rng = np.random.default_rng(11)
    n, f, cx, cy = 600, 700.0, 640.0, 360.0
    from openvo_amd import calib
    R = calib.rodrigues_vec_to_mat([0.01, 0.04, -0.02])
    t = np.array([0.3, -0.05, 0.1])
    X = np.c_[rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), rng.uniform(4, 30, n)]
    X2 = X @ R.T + t
    p1 = np.c_[f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy] + rng.normal(scale=0.2, size=(n, 2))
    p2 = np.c_[f * X2[:, 0] / X2[:, 2] + cx, f * X2[:, 1] / X2[:, 2] + cy] + rng.normal(scale=0.2, size=(n, 2))
    bad = rng.choice(n, n * 4 // 10, replace=False)                      # 40 % outliers
    p2[bad] += rng.uniform(-90, 90, size=(len(bad), 2))
    r5 = oracle.ransac_essential(p1.astype(np.float32), p2.astype(np.float32), [f, f, cx, cy], 400, 1.0, 99, solver=5)
    r8 = oracle.ransac_essential(p1.astype(np.float32), p2.astype(np.float32), [f, f, cx, cy], 400, 1.0, 99, solver=8)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Et = tx @ R
    Et /= np.linalg.norm(Et)
    E5 = r5["E"] / np.linalg.norm(r5["E"])
    assert min(np.abs(E5 - Et).max(), np.abs(E5 + Et).max()) < 0.03
    good = np.setdiff1d(np.arange(n), bad)
    assert r5["mask"][good].mean() > 0.9 and r5["mask"][bad].mean() < 0.1
    # five all-inlier samples are far likelier than eight: more hypotheses land near the winner's inlier count
    assert (r5["counts"] > 0.8 * r5["best_count"]).sum() > (r8["counts"] > 0.8 * r8["best_count"]).sum()
    assert r5["best_count"] >= r8["best_count"] - 5


def test_big_pair_generator_is_reproducible_and_small_case_recovers_the_ground_plane(oracle):
    """tests/big_pair.py builds the 4K frames of the oracle-derived fixtures (tests/golden/o1_sgbm_4k.npz, o2_orb_4k.npz) from
    integer arithmetic: the bytes those fixtures were made from are pinned here by digest, so that a change of the generator
    (or of numpy's integer semantics) shows up on the CPU and not as a mismatch on the GPU box; on a small frame of the same
    generator the oracle's SGBM recovers the scene's disparity law."""
    import hashlib
    from tests.big_pair import pair
    L, R, d = pair(3840, 2160)
    assert hashlib.sha256(L.tobytes()).hexdigest() == "32e5e7208b5d52d6161dfd302f0d267320b1663196ae06b2741c27d6ae498d4f"
    assert hashlib.sha256(R.tobytes()).hexdigest() == "f591efe46274ea2ecd93bba926d0825d867f20226c6b1d5acf23728ced84bffa"
    L2, _, _ = pair(3840, 2160, seed=11)
    assert hashlib.sha256(L2.tobytes()).hexdigest() == "379a5d8dd20d1b1ed6eb3872ff4fca99b12b68bd9343cf885dd1b0de7ddeedbf"
    Ls, Rs, ds = pair(480, 270, dmin=8, dmax=100)
    p = dict(minDisparity=0, numDisparities=128, blockSize=5, P1=200, P2=800, disp12MaxDiff=1, preFilterCap=63,
             uniquenessRatio=10, speckleWindowSize=100, speckleRange=2)
    disp = oracle.sgbm_compute(Ls, Rs, p, 0)
    for y in (20, 135, 250):
        v = disp[y][disp[y] >= 0] / 16.0
        assert len(v) > 100 and abs(np.median(v) - ds[y]) < 0.75
