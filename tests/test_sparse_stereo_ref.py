"""Sparse stereo depth on the CPU: known answers for the numpy restatement (tests/sparse_stereo_ref.py), the restatement on the
oracle's ORB of C1 against the oracle's SGBM, the CPU odometer chain built on it, and the host logic of the new public arguments."""
import os
import re

import numpy as np
import pytest

import sparse_stereo_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (4, 100, 2.0, 75)


def _texture(seed, h=64, w=96):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _kps(xs, ys, octave=0, seed=0):
    n = len(xs)
    return (np.stack([np.asarray(xs, np.float32), np.asarray(ys, np.float32)], 1), np.full(n, octave, np.int32),
            np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8))


# ---- a. known answers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 8, 19])
def test_shifted_copy_gives_the_shift(d):
    """A random texture and its copy shifted by d pixels.  SAD(0) = 0 at the true shift, so s* = 0 and the integer part of the
    disparity is d at EVERY accepted keypoint, exactly.  The parabola term delta = (SAD(-1) - SAD(+1)) / (2 (SAD(-1) + SAD(+1))) of the
    definition is not zero on a texture without symmetry (|delta| < 1/2 follows from SAD(+-1) > 0): there rint(disparity) == d.  On
    a texture that is mirror-symmetric about the keypoint's column SAD(-1) == SAD(+1) term by term, delta = 0 and the disparity
    is d itself, bit for bit."""
    L = _texture(d)
    R = np.roll(L, -d, axis=1)                                   # a point at column x of L lies at column x - d of R
    xs, ys = np.arange(40, 80, 3), np.tile([8, 30, 55], 5)[:14]
    xy, octv, desc = _kps(xs, ys)
    xy_r = xy - np.array([d, 0], np.float32)
    match = S.associate(xy, octv, desc, xy_r, octv, desc, *PARAMS)
    assert np.array_equal(match, np.arange(len(xy)))
    disp = S.refine(L, R, xy, xy_r, match, 4, 100)
    assert not np.isnan(disp).any()
    assert np.array_equal(np.rint(disp), np.full(len(xy), d, np.float32)) and (np.abs(disp - d) < 0.5).all()
    # mirror-symmetric about column 48: keypoints on the axis
    half = _texture(100 + d)[:, :48]
    Ls = np.concatenate([half, np.zeros((64, 1), np.uint8), half[:, ::-1]], axis=1)[:, :96]      # Ls[:, 48 + k] == Ls[:, 48 - k]
    assert np.array_equal(Ls[:, 48 + 5], Ls[:, 48 - 5])
    Rs = np.roll(Ls, -d, axis=1)
    xy, octv, desc = _kps([48, 48, 48], [10, 31, 50])
    xy_r = xy - np.array([d, 0], np.float32)
    match = S.associate(xy, octv, desc, xy_r, octv, desc, *PARAMS)
    disp = S.refine(Ls, Rs, xy, xy_r, match, 4, 100)
    assert np.array_equal(disp.view(np.uint32), np.full(3, d, np.float32).view(np.uint32))


def test_flat_patch_is_rejected():
    L = np.full((64, 96), 90, np.uint8)
    assert np.isnan(S.refine_one(L, L.copy(), 50, 30, 40, 4, 100))           # every SAD is 0: den = 0
    # constant along x only: still den = 0
    L = np.repeat(_texture(3)[:, :1], 96, axis=1)
    assert np.isnan(S.refine_one(L, L.copy(), 50, 30, 40, 4, 100))


def test_minimum_at_the_end_of_the_slide_is_rejected():
    L = _texture(5)
    for off in (-5, 5):
        R = np.roll(L, -(10 + off), axis=1)                       # the true match lies `off` columns from the associated keypoint
        assert np.isnan(S.refine_one(L, R, 60, 30, 50, 4, 100)), off
    R = np.roll(L, -(10 + 4), axis=1)                             # one column inside the slide: kept (s* = -4)
    d = S.refine_one(L, R, 60, 30, 50, 4, 100)
    assert np.rint(d) == 14


def test_two_equal_minima_resolve_to_the_first():
    """The right strip holds the left patch twice, 3 columns apart: SAD = 0 at s = -2 and s = +1; s* is the first."""
    L = _texture(7)
    R = _texture(8)
    x0, y0, xr = 50, 30, 40
    patch = L[y0 - 5:y0 + 6, x0 - 5:x0 + 6]
    # period-3 patch so that the two copies overlap consistently
    p3 = np.tile(patch[:, :3], (1, 8))
    L[y0 - 5:y0 + 6, x0 - 5:x0 + 6] = p3[:, :11]
    R[y0 - 5:y0 + 6, xr - 2 - 5:xr - 2 - 5 + 14] = p3[:, :14]    # copies at s = -2 and s = +1
    sad = [int(np.abs(L[y0 - 5:y0 + 6, x0 - 5:x0 + 6].astype(int) - R[y0 - 5:y0 + 6, xr + s - 5:xr + s + 6].astype(int)).sum()) for s in range(-5, 6)]
    assert sad[3] == 0 and sad[6] == 0 and min(sad[:3]) > 0
    d = S.refine_one(L, R, x0, y0, xr, 4, 100)
    assert not np.isnan(d) and np.rint(d) == x0 - xr + 2 and abs(float(d) - 12) < 0.5
    # ... and association ties go to the lower right index
    xy, octv, desc = _kps([50], [30])
    m = S.associate(xy, octv, desc, np.array([[40, 30], [41, 30]], np.float32), [0, 0], np.repeat(desc, 2, 0), *PARAMS)
    assert m[0] == 0


def test_reproject_matches_the_oracle_at_integer_pixels(oracle):
    Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 400.0], [0, 0, 1 / 0.12, 0]])
    disp = np.zeros((20, 30), np.float32)
    xy = np.array([[3, 4], [10, 7], [29, 19]], np.float32)
    d = np.array([5.25, 17.0, 63.9375], np.float32)
    for (x, y), v in zip(xy.astype(int), d):
        disp[y, x] = v
    want = oracle.reproject_to_3d(disp, Q)
    got = S.reproject(Q, xy, 0, 0, d)
    assert np.array_equal(got, np.stack([want[int(y), int(x)] for x, y in xy]))
    assert np.array_equal(S.reproject(Q, xy - np.float32(2), 2, 2, d), got)       # the ROI origin is a float32 add


# ---- b / c. C1 frames 0-7 -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(oracle):
    from openvo_amd import calib
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    Q, roi = calib.stereo_rectify(c.K(), c.dist(), c.K(), c.dist(), (c.w, c.h), c.rect_params()["R"], c.rect_params()["T"])[4:6]
    frames = c.pairs(0, 8)
    cache = {}
    odo = S.SparseRefOdometer(oracle, Q, roi, frames=cache, pose_method="pnp")
    chain = [(odo.update(L, R), odo.skip_cause, odo.c_T_w.copy()) for L, R in frames]
    return dict(c=c, Q=Q, roi=roi, frames=frames, sparse=[cache[id(L)] for L, _ in frames], chain=chain, odo=odo)


def test_c1_depths_against_the_oracle_sgbm(oracle, c1):
    """Per frame: at least 200 of the 500 keypoints are kept; against the oracle's SGBM disparity at the rint pixel, where that is
    valid, the median |difference| is at most 0.1 px and at most 1 % differ by more than 1 px."""
    c, roi = c1["c"], c1["roi"]
    x0, y0, _, _ = S.crop_bounds(roi, c.w, c.h)
    for k, ((L, R), f) in enumerate(zip(c1["frames"], c1["sparse"])):
        disp16 = oracle.sgbm_compute(L, R, c.sgbm_params())
        px = np.rint(f["xy"]).astype(int) + [x0, y0]
        dense = disp16[px[:, 1], px[:, 0]].astype(np.float32) / 16
        valid = (dense >= 4) & (dense <= 100)
        diff = np.abs(f["disp"][valid] - dense[valid])
        print("frame %d: %d left keypoints, %d accepted, %d kept; %d with a dense disparity: median %.4f px, p90 %.4f, max %.3f" % (
            k, *f["counts3"], valid.sum(), np.median(diff), np.percentile(diff, 90), diff.max()))
        assert f["counts3"][2] >= 200, (k, f["counts3"])
        assert valid.sum() >= 150
        assert np.median(diff) <= 0.1, (k, np.median(diff))
        assert (diff > 1).mean() <= 0.01, (k, (diff > 1).sum())


def test_c1_cpu_chain_end_point(oracle, c1):
    """The CPU chain (restatement + oracle kNN-2, ratio test, P3P RANSAC (256, 1.5, 4321) + gates) over frames 0-7: its end-point
    error is at most one fifth of the dense default odometer's 1.303 m from the same frames."""
    from openvo_amd.synth import Corridor
    from oracle.odometer import RefStereoCamera, RefStereoOdometer
    c, frames = c1["c"], c1["frames"]
    assert all(ok for ok, _, _ in c1["chain"]), [(ok, cause) for ok, cause, _ in c1["chain"]]
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(frames) - 1)
    e_sparse = float(np.linalg.norm(c1["odo"].current_pose()[:3, 3] - gt[:3, 3]))
    dense = RefStereoOdometer(RefStereoCamera(c1["Q"], c1["roi"], c.sgbm_params()), preprocessed_frames=True)
    for L, R in frames:
        dense.update(L, R)
    e_dense = float(np.linalg.norm(dense.current_pose()[:3, 3] - gt[:3, 3]))
    print("end-point error over 7 pairs: dense default %.3f m, sparse + PnP %.3f m" % (e_dense, e_sparse))
    assert abs(e_dense - 1.303) < 5e-3
    assert e_sparse <= 1.303 / 5, e_sparse


# ---- d. host logic --------------------------------------------------------------------------------------------------------------
class _Cam:
    _ctx = None


def test_odometer_validates_the_sparse_arguments():
    from openvo_amd import StereoOdometer
    odo = StereoOdometer(_Cam(), depth="sparse", sparse_row_tol=1.5, sparse_max_hamming=60)
    assert (odo.depth, odo.sparse_row_tol, odo.sparse_max_hamming) == ("sparse", 1.5, 60)
    assert StereoOdometer(_Cam()).depth == "dense"
    for bad in ("Sparse", "", None, 1, True):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth=bad)
    for bad in (-0.5, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="sparse", sparse_row_tol=bad)
    for bad in (-1, 257, 75.0, "75", None, True):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="sparse", sparse_max_hamming=bad)
    assert StereoOdometer(_Cam(), sparse_row_tol=0, sparse_max_hamming=256).sparse_max_hamming == 256


def test_compute_sparse_refuses_a_submitted_pair():
    from openvo_amd.stereo_camera import StereoCamera, SubmittedPair
    cam = StereoCamera.__new__(StereoCamera)              # no device: the refusal comes before anything touches the context
    with pytest.raises(ValueError, match="SubmittedPair"):
        cam.compute_sparse(SubmittedPair(3, (64, 48), True), None, 500)


def test_symbols_and_header_lines():
    from openvo_amd import _native
    header = open(os.path.join(ROOT, "include", "vo355.h")).read()
    for name in ("vo_sparse_stereo", "vo_download_keypoint_depth", "vo_sparse_match_host"):
        assert name in _native.SYMBOLS
        assert re.search(r"^int %s\(vo_ctx\* ctx," % name, header, re.M), name
    for method in ("sparse_stereo", "download_keypoint_depth", "sparse_match_host"):
        assert callable(getattr(_native.Context, method))
    if os.path.exists(_native.LIB_PATH):
        lib = _native.lib()
        for name in ("vo_sparse_stereo", "vo_download_keypoint_depth", "vo_sparse_match_host"):
            assert hasattr(lib, name), name
