"""The numpy restatement of the Lucas-Kanade tracker (tests/klt_ref.py) held to what a tracker must do: identity, the pyramid's
definition, known shifts of a planted texture, each status bit planted, the committed fixture, and the figures DESIGN 4k quotes.
CPU only; the kernels are then held to the restatement bit for bit (tests/test_gpu_klt.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_cases as C                      # noqa: E402
import klt_ref as K                        # noqa: E402


# ---- identity -------------------------------------------------------------------------------------------------------------------------
def test_identity_returns_the_input_exactly():
    a = K.smooth_texture(160, 120, seed=C.SMOOTH_SEED)
    xy = np.stack(np.meshgrid(np.arange(25, 135, 10), np.arange(25, 95, 10)), -1).reshape(-1, 2).astype(np.float32)
    for pts in (xy, xy + np.float32(0.37)):
        out, st, it = K.track(a, a, pts)
        assert (st == 0).all() and C.same_bits(out, pts)
        assert (it >= 1).all()                                    # (it looked: one iteration per level that has texture)


# ---- pyramid --------------------------------------------------------------------------------------------------------------------------
def test_pyramid_sizes_constant_and_a_hand_computed_corner():
    rng = np.random.default_rng(0)
    for (w, h), sizes in (((97, 65), [(65, 97), (33, 49), (17, 25), (9, 13)]), ((96, 64), [(64, 96), (32, 48), (16, 24), (8, 12)])):
        p = K.pyramid(rng.integers(0, 256, (h, w)).astype(np.uint8), 4)
        assert [l.shape for l in p] == sizes and all(l.dtype == np.uint8 for l in p)
    for v in (0, 1, 77, 254, 255):
        assert all((l == v).all() for l in K.pyramid(np.full((65, 97), v, np.uint8), 4))
    img = (np.arange(5)[:, None] * 10 + np.arange(6)[None, :] * 3 + 1).astype(np.uint8)          # 5 rows x 6 columns
    # img[r][c] = 10 r + 3 c + 1 is linear, so a weighted sum is 256 (10 E[r] + 3 E[c] + 1) with the mean index under the weights.
    # pixel (0, 0): indices -2 .. 2 reflect to 2 1 0 1 2, weights 6 / 8 / 2 on 0 / 1 / 2, mean 12 / 16 = 0.75 in both directions:
    # 256 * (7.5 + 2.25 + 1) = 2752, (2752 + 128) >> 8 = 11
    wt = np.array([6, 8, 2])
    want = (int((wt[:, None] * wt[None, :] * img[:3, :3].astype(np.int64)).sum()) + 128) >> 8
    got = K.pyr_down(img)
    assert got.shape == (3, 3) and int(got[0, 0]) == want == 11
    # pixel (2, 2), the far corner: rows 2 .. 6 of 5 reflect to 2 3 4 3 2 (weights 2 / 8 / 6 on 2 / 3 / 4, mean 3.25), columns 2 .. 6 of 6
    # to 2 3 4 5 4 (weights 1 / 4 / 7 / 4 on 2 .. 5, mean 3.875): 256 * (32.5 + 11.625 + 1) = 11552, (11552 + 128) >> 8 = 45
    wr, wc = np.array([0, 0, 2, 8, 6]), np.array([0, 0, 1, 4, 7, 4])
    assert int(got[2, 2]) == (int((wr[:, None] * wc[None, :] * img.astype(np.int64)).sum()) + 128) >> 8 == 45


def test_gradient_of_a_ramp():
    """Scharr of I = 2 x + 3 y is (32 * 2, 32 * 3) inside and sees the clamped reads at the border"""
    img = (2 * np.arange(20)[None, :] + 3 * np.arange(12)[:, None]).astype(np.uint8)
    Dx, Dy = K.scharr(img)
    assert Dx.shape == (14, 22) and (Dx[2:-2, 2:-2] == 64).all() and (Dy[2:-2, 2:-2] == 96).all()
    assert (Dx[2:-2, 0] == 0).all() and (Dx[2:-2, 1] == 32).all() and (Dy[0, 2:-2] == 0).all()     # x = -1: both reads clamp to column 0


# ---- known shifts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ((2.5, -1.25), (7.0, 3.0)))
@pytest.mark.parametrize("w,h,win,levels", ((160, 120, 21, 3), (96, 64, 9, 2)))
def test_known_shift_of_the_smooth_texture(w, h, win, levels, shift):
    """every point tracked, forward-backward distance <= 0.01 px, error <= 0.1 px"""
    a, b = C.smooth_pair(w, h, shift, flat=False)
    m = win + max(abs(shift[0]), abs(shift[1])) + 2
    rng = np.random.default_rng(1)
    xy = np.stack([rng.uniform(m, w - 1 - m, 200), rng.uniform(m, h - 1 - m, 200)], 1).astype(np.float32)
    out, st, it = K.track(a, b, xy, win=win, levels=levels, fb=0.01)
    back, stb, _ = K.track(b, a, out, win=win, levels=levels, fb=0)
    err = np.abs(out.astype(np.float64) - (xy.astype(np.float64) - np.array(shift))).max(axis=1)       # (content at p is at p - shift in b)
    d = np.sqrt(((back.astype(np.float64) - xy) ** 2).sum(axis=1))
    print("%dx%d win %d levels %d shift %s: error max %.4f px, forward-backward max %.4f px, iterations %d .. %d"
          % (w, h, win, levels, shift, err.max(), d.max(), it.min(), it.max()))
    assert (st == 0).all() and (stb == 0).all()
    assert d.max() <= 0.01
    assert err.max() <= 0.1


# ---- status bits, each planted --------------------------------------------------------------------------------------------------------
def test_status_bits():
    w, h = 160, 120
    a, b = C.smooth_pair(w, h)                                      # shift (2.5, -1.25), flat patch in both
    F = C.flat_rect(w, h)
    flat = (F[0] + F[2] / 2.0, F[1] + F[3] / 2.0)
    xy = np.array([flat, (80.5, 100.25), (np.nan, 5.0), (5.0, -np.inf)], np.float32)
    out, st, it = K.track(a, b, xy, win=21, levels=3)
    assert st[0] == K.ST_EIG and it[0] >= 0
    assert st[1] == 0
    assert st[2] == st[3] == K.ST_NONFINITE and it[2] == it[3] == 0 and C.same_bits(out[2:], xy[2:])
    # flow that leaves the image: content near the left border moves out by 7 px
    a2, b2 = C.smooth_pair(w, h, (7.0, 0.0), flat=False)
    out, st, _ = K.track(a2, b2, np.array([(3.0, 60.0), (80.0, 60.0)], np.float32), win=21, levels=3, fb=0)
    assert st[0] == K.ST_OUT and out[0, 0] < 0 and st[1] == 0
    # a point far outside is lost in the iteration, wherever its template happened to land
    out, st, it = K.track(a2, b2, np.array([(-500.0, 60.0), (3.0e38, 0.0)], np.float32), win=21, levels=3, fb=0)
    assert (st & K.ST_OUT).all() and (it == 0).all()
    # occlusion: in b the patch around the point is replaced by other texture, the backward track lands elsewhere
    a3, b3 = C.smooth_pair(w, h, (0.0, 0.0), flat=False)
    b3 = b3.copy()
    b3[40:80, 60:100] = K.smooth_texture(40, 40, seed=99)
    pts = np.array([(80.0, 60.0), (30.0, 30.0)], np.float32)
    out0, st0, _ = K.track(a3, b3, pts, win=21, levels=3, fb=0)
    out, st, it = K.track(a3, b3, pts, win=21, levels=3, fb=1.0)
    assert st0[0] == 0 and st[0] == K.ST_FB and st[1] == 0 and C.same_bits(out, out0)
    assert it[1] > K.track(a3, b3, pts, win=21, levels=3, fb=0)[2][1]          # (the backward pass counts too)


def test_parameter_rules():
    a = K.smooth_texture(32, 32)
    for kw in (dict(win=4), dict(win=6), dict(win=33), dict(levels=0), dict(levels=7), dict(iters=0), dict(iters=101), dict(eps=-1),
               dict(min_eig=float("nan")), dict(fb=float("inf")), dict(win=True), dict(levels=2.0)):
        with pytest.raises(ValueError):
            K.track(a, a, np.zeros((1, 2), np.float32), **kw)
    out, st, it = K.track(a, a, np.zeros((0, 2), np.float32))
    assert out.shape == (0, 2) and st.shape == it.shape == (0,)


# ---- the committed fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_corridor_crop_and_oscillates():
    a, b, osc = C.fixture()
    ra, rb = C.corridor_crops()
    assert np.array_equal(a, ra) and np.array_equal(b, rb) and a.shape == (120, 160)
    assert len(osc) >= 4 and np.array_equal(osc, C.find_oscillating(a, b)[:8])
    tr = {}
    out, st, it = K.track(a, b, osc, fb=0, trace=tr, **C.OSC_PARAMS)
    assert (tr["osc"] > 0).all() and (st == 0).all()
    # the iteration counts vary on the corridor, as the issue's prototype saw
    xy = C.points(160, 120, 257)
    _, st, it = K.track(a, b, xy, win=21, levels=3, fb=0)
    print("corridor T0 crop, win 21 / 3 levels: iterations %d .. %d over %d tracked points" % (it[st == 0].min(), it[st == 0].max(), (st == 0).sum()))
    assert it[st == 0].max() >= 3 * it[st == 0].min()


# ---- what it buys: recorded, asserted only for sanity ---------------------------------------------------------------------------------
def test_corridor_c1_klt_pnp_against_the_descriptor_chain(oracle):
    """C1 frames 0 - 7, sparse stereo depth, PnP with 4 RANSAC seeds: end-point error of the tracked chain beside the descriptor
    chain's, and the tracks kept per pair.  Printed (DESIGN 4k quotes it whichever way it falls); asserted: every frame accepted and
    the error below the default descriptor odometer's 1.303 m."""
    import klt_chain_ref as KC
    import sparse_stereo_ref as S
    from openvo_amd import calib
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    Q, roi = calib.stereo_rectify(c.K(), c.dist(), c.K(), c.dist(), (c.w, c.h), c.rect_params()["R"], c.rect_params()["T"])[4:6]
    frames = c.pairs(0, 8)
    gt = np.linalg.inv(type(c).gt_pose(0)) @ type(c).gt_pose(7)
    cache, tracks = {}, {}
    rows = []
    for seed in (4321, 1, 2, 3):
        k = KC.KltSparseRefOdometer(oracle, Q, roi, nfeatures=500, pnp_seed=seed, frames=cache, tracks=tracks, klt=dict(K.DEFAULTS))
        d = S.SparseRefOdometer(oracle, Q, roi, nfeatures=500, pose_method="pnp", pnp_seed=seed, frames=cache)
        ok_k = [k.update(L, R) for L, R in frames]
        ok_d = [d.update(L, R) for L, R in frames]
        e_k = float(np.linalg.norm(np.linalg.inv(k.c_T_w)[:3, 3] - gt[:3, 3]))
        e_d = float(np.linalg.norm(np.linalg.inv(d.c_T_w)[:3, 3] - gt[:3, 3]))
        rows.append((seed, e_k, e_d, all(ok_k), all(ok_d), list(k.kept)))
        print("seed %4d: KLT + PnP %.4f m, descriptors + PnP %.4f m (accepted %d / %d of 8); tracks kept per pair %s"
              % (seed, e_k, e_d, sum(ok_k), sum(ok_d), " ".join("%d/%d" % (b, a) for a, b in k.kept)))
    for seed, e_k, e_d, all_k, _, kept in rows:
        assert all_k and e_k < 1.303, (seed, e_k)
        assert len(kept) == 7
