"""The association tests of the sparse stereo chain (vo_set_sparse_assoc: mutual, ratio) and the right partners' descriptors
(kp_rdesc) on the GPU, against the numpy restatement tests/sparse_loop_ref.py: k_sparse_pair alone through the host seam
vo_sparse_pair_host_ex (96 x 64 images, match equal, every float as its bit pattern), vo_sparse_stereo and its look-ahead entries
under each association state on C1 / T0 frames, and StereoOdometer(sparse_mutual=, sparse_ratio=) against the CPU chain.  All on
ctx_small (kp_cap 3024: every launch has 756 workgroups, most of which only draw a ticket)."""
import numpy as np
import pytest

import sparse_loop_ref as X
import sparse_stereo_ref as S
from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

H, W = 64, 96
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
P = dict(min_disp=4, max_disp=40, row_tol=2.0, max_hamming=75)
Q = np.array([[1, 0, 0, -48.0], [0, 1, 0, -32.0], [0, 0, 0, 80.0], [0, 0, 1.0 / 0.12, 0]], np.float64)
ROI_XY = (7, 3)
STATES = ((False, None), (True, None), (False, 0.8), (True, 0.8))          # flags 0, 1, 2, 3
PARAMS = (4, 100, 2.0, 75)
KP = ("xy", "size", "angle", "response", "octave", "desc")


def _fl(mutual, ratio):
    return (X.MUTUAL if mutual else 0) | (X.RATIO if ratio is not None else 0)


def _flip(d, nbits, rng):
    u = np.unpackbits(np.asarray(d, np.uint8).reshape(32))
    u[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(u)


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32) | (np.isnan(a) * np.uint32(0x7FFFFFFF))       # (every NaN is one pattern)


def _kpd(k):
    n = len(k[0])
    z = np.zeros(n, np.float32)
    return dict(xy=np.asarray(k[0], np.float32).reshape(-1, 2), size=z, angle=z, response=z, octave=np.asarray(k[1], np.int32),
                desc=np.asarray(k[2], np.uint8).reshape(-1, 32))


def _crowded_scene(seed, nl, nr, nb=90):
    """nb world points with a descriptor each; every right and every left keypoint is a noisy view of a random one of them (left
    shifted by the disparity), so several left keypoints want the same right one and most have a close runner-up"""
    rng = np.random.default_rng(seed)
    d = int(rng.integers(6, 20))
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = np.roll(L, -d, axis=1)
    bx = np.stack([rng.uniform(0, W - d, nb), rng.uniform(0, H, nb)], 1)
    bo = rng.integers(0, 8, nb)
    bd = rng.integers(0, 256, (nb, 32), dtype=np.uint8)

    def views(n, shift, noise):
        w = rng.integers(0, nb, n)
        xy = (bx[w] + np.stack([rng.normal(0, 1.0, n) + shift, rng.normal(0, 1.0, n)], 1)).astype(np.float32)
        xy[::3] = np.rint(xy[::3]) + np.float32(0.5)
        o = np.clip(bo[w] + rng.integers(-1, 2, n), 0, 7).astype(np.int32)
        de = np.stack([_flip(bd[k], int(rng.integers(*noise)), rng) for k in w]) if n else np.zeros((0, 32), np.uint8)
        return xy, o, de
    kl = views(nl, d, (0, 50))
    xy_r, o_r, d_r = views(nr, 0, (0, 40))
    order = np.argsort(o_r, kind="stable")
    return L, R, kl, (xy_r[order], o_r[order], d_r[order])


def _check(ctx, L, R, kl, kr, mutual, ratio, **over):
    p = dict(P, **over)
    want = X.sparse_stereo_ex(L, R, _kpd(kl), _kpd(kr), Q, ROI_XY[0], ROI_XY[1], p["min_disp"], p["max_disp"], p["row_tol"], p["max_hamming"],
                              _fl(mutual, ratio), ratio)
    got = ctx.sparse_pair_host(L, R, kl[0], kl[1], kl[2], kr[0], kr[1], kr[2], Q, ROI_XY, mutual=mutual, assoc_ratio=ratio, **p)
    assert np.array_equal(got["counts3"], want["counts3"]), (got["counts3"], want["counts3"])
    assert np.array_equal(got["match"], want["match"])
    assert np.array_equal(_bits(got["disp"]), _bits(want["disp_all"]))
    for k in ("xy", "octave", "desc"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["kp_disp"]), _bits(want["disp"]))
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"]))
    assert np.array_equal(got["rdesc"], want["rdesc"])
    assert np.array_equal(got["rdesc"], np.asarray(kr[2], np.uint8).reshape(-1, 32)[got["match"][want["keep"]]])
    return want


# ---- the seam ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual,ratio", STATES)
def test_every_count_under_every_state(ctx_small, mutual, ratio):
    """0 / 1 / 130 / 400 left against 0 / 1 / 300 right keypoints; at 400 x 300 each enabled test removes associations"""
    for a, nl in enumerate((0, 1, 130, 400)):
        for b, nr in enumerate((0, 1, 300)):
            L, R, kl, kr = _crowded_scene(100 + 10 * a + b, nl, nr)
            want = _check(ctx_small, L, R, kl, kr, mutual, ratio)
            assert want["counts3"][0] == nl
    plain = X.sparse_stereo_ex(L, R, _kpd(kl), _kpd(kr), Q, *ROI_XY, *[P[k] for k in ("min_disp", "max_disp", "row_tol", "max_hamming")])
    print("400 x 300, mutual %s ratio %s: counts3 %s (no test: %s)" % (mutual, ratio, want["counts3"], plain["counts3"]))
    assert plain["counts3"][1] >= 150 and want["counts3"][2] >= 10
    if mutual or ratio is not None:
        assert want["counts3"][1] < plain["counts3"][1]


def test_planted_cases(ctx_small):
    """the known answers of tests/test_sparse_loop_ref.py through the kernel"""
    rng = np.random.default_rng(3)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = np.roll(L, -10, axis=1)
    b0, b1 = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))

    def fl(d, bits):
        u = np.unpackbits(d)
        u[list(bits)] ^= 1
        return np.packbits(u)

    def row(xs):
        return np.stack([np.asarray(xs, np.float32), np.full(len(xs), 30, np.float32)], 1)
    z = lambda n: np.zeros(n, np.int32)
    # two left keypoints with the same best: the smaller distance, then the lower i
    for dl, win in (([fl(b0, range(5)), fl(b0, range(3))], [-1, 0]), ([fl(b0, range(4)), fl(b0, range(4, 8))], [0, -1])):
        w = _check(ctx_small, L, R, (row([50, 52]), z(2), np.stack(dl)), (row([40]), z(1), b0[None]), True, None)
        assert list(w["match"]) == win
    # a better claimant whose winner is elsewhere still defeats the claim
    l1 = fl(b1, range(2))
    r0 = fl(l1, range(10, 14))
    l0 = fl(r0, range(20, 30))
    w = _check(ctx_small, L, R, (row([50, 60]), z(2), np.stack([l0, l1])), (row([45, 55]), z(2), np.stack([r0, b1])), True, None)
    assert list(w["match"]) == [-1, 1]
    # ratio: d1 == d2 fails at 1; a single candidate passes; a runner-up above max_hamming still counts
    two = (row([50, 48]), z(2), np.stack([fl(b0, range(6)), fl(b0, range(6, 12))]))
    assert list(_check(ctx_small, L, R, (row([60]), z(1), b0[None]), two, False, 1.0)["match"]) == [-1]
    assert list(_check(ctx_small, L, R, (row([60]), z(1), b0[None]), (two[0][:1], two[1][:1], two[2][:1]), False, 0.5)["match"]) == [0]
    far = (row([50, 48]), z(2), np.stack([fl(b0, range(70)), fl(b0, range(100, 180))]))
    assert list(_check(ctx_small, L, R, (row([60]), z(1), b0[None]), far, False, 0.8)["match"]) == [-1]
    assert list(_check(ctx_small, L, R, (row([60]), z(1), b0[None]), far, False, None)["match"]) == [0]


def test_every_left_keypoint_claims_the_same_right_one(ctx_small):
    """130 left keypoints in one row band, one right keypoint within reach of all (and, second, 299 more that nobody can reach):
    with the mutual test exactly one of them keeps it -- the nearest, the lowest index among equals"""
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W]
    L = (127 + 60 * np.sin(xx * 0.35) + 50 * np.cos(yy * 0.4 + xx * 0.05)).astype(np.uint8)
    R = np.roll(L, -10, axis=1)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    n = 130
    xy_l = np.stack([rng.uniform(40, 60, n), rng.uniform(29.5, 30.5, n)], 1).astype(np.float32)
    d_l = np.stack([_flip(base, int(rng.integers(5, 60)), rng) for _ in range(n)])
    d_l[7] = d_l[90] = _flip(base, 3, rng)                       # two equal nearest claimants: index 7 wins
    kl = (xy_l, np.zeros(n, np.int32), d_l)
    for nr in (1, 300):
        xy_r = np.concatenate([[[30.0, 30.0]], np.stack([rng.uniform(0, W, nr - 1), rng.uniform(50, 64, nr - 1)], 1)]).astype(np.float32)
        kr = (xy_r, np.zeros(nr, np.int32), np.concatenate([base[None], rng.integers(0, 256, (nr - 1, 32), dtype=np.uint8)]))
        w = _check(ctx_small, L, R, kl, kr, True, None)
        assert w["counts3"][1] == 1 and list(np.nonzero(w["match"] >= 0)[0]) == [7]
        assert _check(ctx_small, L, R, kl, kr, False, None)["counts3"][1] == n
        assert _check(ctx_small, L, R, kl, kr, True, 0.8)["counts3"][1] == 1


@pytest.mark.parametrize("mutual,ratio", STATES[1:])
def test_nothing_kept_and_everything_kept(ctx_small, mutual, ratio):
    L, R, kl, kr = _crowded_scene(77, 300, 300)
    noise = np.random.default_rng(1).integers(0, 256, (300, 32), dtype=np.uint8)
    want = _check(ctx_small, L, R, kl, (kr[0], kr[1], noise), mutual, ratio, max_hamming=0)
    assert list(want["counts3"]) == [300, 0, 0]
    yy, xx = np.mgrid[0:H, 0:W]
    L = (127 + 60 * np.sin(xx * 0.35) + 50 * np.cos(yy * 0.4 + xx * 0.05)).astype(np.uint8)
    R = np.roll(L, -10, axis=1)
    n = 260
    rng = np.random.default_rng(5)
    xy_l = np.stack([rng.integers(30, W - 8, n), rng.integers(6, H - 6, n)], 1).astype(np.float32)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)               # distinct descriptors: each finds its own twin at distance 0
    o = np.sort(rng.integers(0, 8, n)).astype(np.int32)
    want = _check(ctx_small, L, R, (xy_l, o, d), (xy_l - np.array([10, 0], np.float32), o, d), mutual, ratio, max_hamming=0, row_tol=0.0)
    assert list(want["counts3"]) == [n, n, n]


def test_five_calls_back_to_back_with_alternating_states(ctx_small):
    """the launch that used the claim words puts them back: a word left behind would defeat a claim of the next mutual launch
    (and the launches without the test must not care)"""
    total = 0
    for k, (nl, nr, st) in enumerate(((400, 300, 3), (130, 300, 0), (400, 300, 1), (300, 1, 2), (400, 300, 1))):
        total += int(_check(ctx_small, *_crowded_scene(900 + k, nl, nr), *STATES[st])["counts3"][2])
    assert total >= 60


def test_hostile_association_arguments_return_a_status(ctx_small):
    L, R, kl, kr = _crowded_scene(7, 10, 10)
    for mutual, ratio in ((False, 0.8), (True, None)):
        _check(ctx_small, L, R, kl, kr, mutual, ratio)
    lib, h, p = ctx_small._lib, ctx_small._h, _native._p
    m, d = np.zeros(10, np.int32), np.zeros(10, np.float32)
    xy, o, de, kd, xyz = np.zeros((10, 2), np.float32), np.zeros(10, np.int32), np.zeros((10, 32), np.uint8), np.zeros(10, np.float32), np.zeros((10, 3), np.float32)
    rd, c3, Qc = np.zeros((10, 32), np.uint8), np.zeros(3, np.int32), np.ascontiguousarray(Q.reshape(16))

    def call(flags, ratio, rdesc=rd):
        return lib.vo_sparse_pair_host_ex(h, p(L), p(R), W, H, p(kl[0]), p(kl[1]), p(kl[2]), 10, p(kr[0]), p(kr[1]), p(kr[2]), 10, 4.0, 40.0, 2.0, 75,
                                          flags, ratio, p(Qc), 7, 3, p(m), p(d), p(xy), p(o), p(de), p(kd), p(xyz), p(rdesc), p(c3))
    assert call(0, 0.0) == 0 and call(1, float("nan")) == 0 and call(3, 1.0) == 0 and call(0, 0.0, None) == 0
    for flags, ratio in ((4, 0.5), (-1, 0.5), (2, 0.0), (2, -0.5), (3, 1.5), (2, float("nan")), (2, float("inf"))):
        assert call(flags, ratio) == VO_E_ARG, (flags, ratio)
        assert lib.vo_set_sparse_assoc(h, flags, ratio) == VO_E_ARG, (flags, ratio)
    assert lib.vo_set_sparse_assoc(None, 0, 0.0) == VO_E_ARG
    _check(ctx_small, L, R, kl, kr, True, 0.8)


# ---- vo_sparse_stereo under each state ---------------------------------------------------------------------------------------------
def _camera(ctx, name):
    c = Corridor(name)
    return c, StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)


def _slot_arrays(ctx, slot):
    got = ctx.download_keypoints(slot)
    got["xyz"], got["disp"] = ctx.download_keypoint_depth(slot)
    got["rdesc"] = ctx.download_keypoint_rdesc(slot)
    return got


def _same(got, want):
    for k in KP + ("rdesc",):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["disp"]), _bits(want["disp"])) and np.array_equal(_bits(got["xyz"]), _bits(want["xyz"]))


@pytest.fixture(scope="module")
def rig(ctx_small):
    """two C1 frames (500 features) and one T0 frame (300): per frame and association state the restatement on the library's own
    ORB of the two crops (computed once, the ORB once per frame)"""
    ctx = ctx_small
    out = []
    try:
        for name, k, nf in (("C1", 0, 500), ("C1", 1, 500), ("T0", 0, 300)):
            c, cam = _camera(ctx, name)
            Lf, Rf = c.pairs(k, k + 1)[0]
            x0, y0, x1, y1 = S.crop_bounds(cam.valid_region_left, c.w, c.h)
            Lc, Rc = np.ascontiguousarray(Lf[y0:y1, x0:x1]), np.ascontiguousarray(Rf[y0:y1, x0:x1])
            kl, kr = ctx.orb_host(Lc, None, nf), ctx.orb_host(Rc, None, nf)
            want = [X.sparse_stereo_ex(Lc, Rc, kl, kr, cam.Q, x0, y0, *PARAMS, _fl(*st), st[1]) for st in STATES]
            out.append(dict(name=name, cam=cam, pair=(Lf, Rf), nf=nf, want=want))
        yield out
    finally:
        ctx.set_sparse_assoc(False, None)


def _use(ctx, f):
    """the frame's camera settings into the shared context"""
    ctx.set_Q(f["cam"].Q)
    ctx.set_roi(*f["cam"].valid_region_left)


def test_sparse_stereo_under_each_state(ctx_small, rig):
    ctx = ctx_small
    ctx.upload_pair(20, *rig[0]["pair"], True)
    with pytest.raises(_native.VoError) as e:
        ctx.download_keypoint_rdesc(20)                                     # (a pair, no sparse result)
    assert e.value.code == VO_E_STATE
    for f in rig:
        _use(ctx, f)
        ctx.upload_pair(3, *f["pair"], True)
        for st, want in zip(STATES, f["want"]):
            ctx.set_sparse_assoc(*st)
            c3 = ctx.sparse_stereo(3, f["nf"], *PARAMS)
            print("%s, mutual %s ratio %s: counts3 %s" % (f["name"], st[0], st[1], c3))
            assert np.array_equal(c3, want["counts3"]), (c3, want["counts3"])
            _same(_slot_arrays(ctx, 3), want)
        assert f["want"][3]["counts3"][1] < f["want"][0]["counts3"][1] and f["want"][3]["counts3"][2] >= 30
    ctx.set_sparse_assoc(False, None)


def test_a_chain_begun_ahead_belongs_to_the_state_it_was_begun_under(ctx_small, rig):
    """begun under one state and collected under another: recomputed (one launch of the association on the main stream); begun
    and collected under the same: nothing is launched, and the result is the synchronous call's"""
    ctx, f = ctx_small, rig[0]
    _use(ctx, f)
    f["cam"].stage_pairs([f["pair"]])
    try:
        for begun, collected in ((3, 3), (3, 0), (0, 1), (2, 2), (1, 3)):
            ctx.set_sparse_assoc(*STATES[begun])
            ctx.prefetch_staged_pair_sparse(5, 0, True, f["nf"], *PARAMS)
            ctx.set_sparse_assoc(*STATES[collected])
            ctx.enable_timing(True, ("match",))
            ctx.timings(reset=True)
            c3 = ctx.sparse_stereo(5, f["nf"], *PARAMS)
            launches = ctx.timings(reset=True)["match"][1]
            ctx.enable_timing(False)
            assert launches == (0 if begun == collected else 1), (begun, collected, launches)
            want = f["want"][collected]
            assert np.array_equal(c3, want["counts3"])
            _same(_slot_arrays(ctx, 5), want)
            assert ctx.lookahead_depth() == 0
            assert np.array_equal(ctx.sparse_stereo(5, f["nf"], *PARAMS), c3)
    finally:
        ctx.enable_timing(False)
        ctx.set_sparse_assoc(False, None)


# ---- the odometer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(rigidity_threshold=0.1, outlier_threshold=0.02), dict(pose_method="pnp")], ids=["default", "clique", "pnp"])
def test_odometer_with_the_association_tests_against_the_cpu_chain(ctx_small, oracle, kw):
    """StereoOdometer(depth="sparse", sparse_mutual=True, sparse_ratio=0.8) over C1 frames 0-7 against the CPU chain on the
    library's ORB: flags, skip_cause, c_T_w to 1e-9; run(depth=4) equals the update() chain exactly; the camera's results carry
    right_desc"""
    ctx = ctx_small
    c, cam = _camera(ctx, "C1")
    frames = c.pairs(0, 8)
    x0, y0, x1, y1 = S.crop_bounds(cam.valid_region_left, c.w, c.h)
    try:
        ref = X.SparseLoopOdometer(oracle, cam.Q, cam.valid_region_left, mutual=True, ratio=0.8, frames={}, **kw)
        for L, R in frames:
            Lc, Rc = np.ascontiguousarray(L[y0:y1, x0:x1]), np.ascontiguousarray(R[y0:y1, x0:x1])
            f = X.sparse_stereo_ex(Lc, Rc, ctx.orb_host(Lc, None, 500), ctx.orb_host(Rc, None, 500), cam.Q, x0, y0, *PARAMS, 3, 0.8)
            f["origin"] = (x0, y0)
            ref.frames[id(L)] = f
        odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", sparse_mutual=True, sparse_ratio=0.8, **kw)
        chain = []
        for L, R in frames:
            ok, want_ok = odo.update(L, R), ref.update(L, R)
            assert (ok, odo.skip_cause) == (want_ok, ref.skip_cause)
            assert np.abs(odo.c_T_w - ref.c_T_w).max() <= 1e-9
            chain.append((ok, odo.c_T_w.copy()))
        assert sum(ok for ok, _ in chain) >= 7
        assert np.array_equal(odo.current_3d.right_desc, ref.cur["rdesc"]) and np.array_equal(np.asarray(odo.current_3d), ref.cur["xyz"])
        odo.reset_lookahead()
        ran = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", sparse_mutual=True, sparse_ratio=0.8, **kw)
        for k, ok in enumerate(ran.run(iter(frames), depth=4)):
            if k == 0:
                assert ctx.lookahead_depth() >= 1                               # pairs were begun ahead, under this state
            assert ok == chain[k][0] and np.array_equal(ran.c_T_w, chain[k][1]), k
        assert ctx.lookahead_depth() == 0
        ran.reset_lookahead()
    finally:
        ctx.set_sparse_assoc(False, None)
