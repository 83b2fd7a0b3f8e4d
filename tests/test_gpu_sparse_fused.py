"""k_sparse_pair alone -- association, refinement and, in the workgroup that arrives last at the ticket, the ordered compaction, in
ONE launch -- through the host seam vo_sparse_pair_host, against the numpy restatement tests/sparse_stereo_ref.py::sparse_stereo:
match equal, every float as its bit pattern.  Context (0, 128, 96, 16, 400): the launch has 456 workgroups whatever the counts
(the product's grid), so with 400 left keypoints 100 of them work and the rest only draw a ticket; 96 x 64 images."""
import numpy as np
import pytest

import sparse_stereo_ref as S
from openvo_amd import _native

pytestmark = pytest.mark.gpu

H, W = 64, 96
VO_E_ARG, VO_E_CAP = -1, -4
P = dict(min_disp=4, max_disp=40, row_tol=2.0, max_hamming=75)
Q = np.array([[1, 0, 0, -48.0], [0, 1, 0, -32.0], [0, 0, 0, 80.0], [0, 0, 1.0 / 0.12, 0]], np.float64)
ROI_XY = (7, 3)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 128, 96, 16, 400)
    yield c
    c.close()


def _texture(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _desc(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(desc, nbits, seed=0):
    """desc with `nbits` distinct bits flipped in every row"""
    out = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1)
    rng = np.random.default_rng(seed)
    for r in out:
        r[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(out, axis=1)


def _random_scene(seed, nl, nr):
    """(as tests/test_gpu_sparse_match.py builds its scenes)"""
    rng = np.random.default_rng(seed)
    d = int(rng.integers(5, 25))
    L = _texture(seed)
    R = np.roll(L, -d, axis=1)
    xy_l = np.stack([rng.uniform(0, W, nl), rng.uniform(0, H, nl)], 1).astype(np.float32)
    xy_l[::3] = np.rint(xy_l[::3]) + np.float32(0.5)            # halves
    o_l = rng.integers(0, 8, nl).astype(np.int32)
    d_l = _desc(nl, seed + 1)
    xy_r = np.stack([rng.uniform(0, W, nr), rng.uniform(0, H, nr)], 1).astype(np.float32)
    o_r = np.sort(rng.integers(0, 8, nr)).astype(np.int32)
    d_r = _desc(nr, seed + 2)
    for j in range(min(nl, nr)):            # right keypoint j answers left keypoint (some i): shifted, jittered, a noisy copy of its descriptor
        i = int(rng.integers(0, nl))
        xy_r[j] = xy_l[i] - np.array([d + rng.normal(0, 1.5), rng.normal(0, 1.5)], np.float32)
        o_r[j] = np.clip(o_l[i] + rng.integers(-2, 3), 0, 7)
        d_r[j] = _flip(d_l[i:i + 1], int(rng.integers(40, 100)), seed + j)[0]
    order = np.argsort(o_r, kind="stable")
    return L, R, (xy_l, o_l, d_l), (xy_r[order], o_r[order], d_r[order])


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32) | (np.isnan(a) * np.uint32(0x7FFFFFFF))       # (every NaN is one pattern: the kernel's and numpy's differ in sign only)


def _kpd(k):
    n = len(k[0])
    z = np.zeros(n, np.float32)
    return dict(xy=np.asarray(k[0], np.float32).reshape(-1, 2), size=z, angle=z, response=z, octave=np.asarray(k[1], np.int32),
                desc=np.asarray(k[2], np.uint8).reshape(-1, 32))


def _check(ctx, L, R, kl, kr, **over):
    p = dict(P, **over)
    want = S.sparse_stereo(L, R, _kpd(kl), _kpd(kr), Q, ROI_XY[0], ROI_XY[1], p["min_disp"], p["max_disp"], p["row_tol"], p["max_hamming"])
    disp_all = S.refine(L, R, _kpd(kl)["xy"], _kpd(kr)["xy"], want["match"], p["min_disp"], p["max_disp"])
    got = ctx.sparse_pair_host(L, R, kl[0], kl[1], kl[2], kr[0], kr[1], kr[2], Q, ROI_XY, **p)
    assert np.array_equal(got["counts3"], want["counts3"]), (got["counts3"], want["counts3"])
    assert np.array_equal(got["match"], want["match"])
    assert np.array_equal(_bits(got["disp"]), _bits(disp_all))
    for k in ("xy", "octave", "desc"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["kp_disp"]), _bits(want["disp"]))
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"]))
    return want


@pytest.mark.parametrize("nr", [0, 1, 300])
def test_every_left_count(ctx, nr):
    """one workgroup with work (1, 4), two (5), a compaction loop that runs twice (257, 300, 400), none at all (0)"""
    kept = 0
    for a, nl in enumerate((0, 1, 4, 5, 64, 257, 300, 400)):
        L, R, kl, kr = _random_scene(500 + 10 * a + nr, nl, nr)
        want = _check(ctx, L, R, kl, kr)
        assert want["counts3"][0] == nl
        kept += int(want["counts3"][2])
    print("nr %d: kept %d over the eight left counts" % (nr, kept))
    assert kept >= (40 if nr == 300 else 0)


def test_five_calls_back_to_back(ctx):
    """the last arriver puts the ticket back: every later launch finds it at zero"""
    total = 0
    for k, (nl, nr) in enumerate(((400, 300), (5, 300), (257, 1), (0, 0), (300, 300))):
        total += int(_check(ctx, *_random_scene(900 + k, nl, nr))["counts3"][2])
    assert total >= 40


def test_nothing_kept_and_everything_kept(ctx):
    # nothing: no right keypoint within max_hamming = 0 of any left one
    L, R, kl, kr = _random_scene(77, 300, 300)
    want = _check(ctx, L, R, kl, kr, max_hamming=0)
    assert want["counts3"][2] == 0 and want["counts3"][0] == 300
    # everything: a smooth texture shifted by 10, every left keypoint on the integer grid well inside, its right twin 10 to the left
    yy, xx = np.mgrid[0:H, 0:W]
    L = (127 + 60 * np.sin(xx * 0.35) + 50 * np.cos(yy * 0.4 + xx * 0.05)).astype(np.uint8)
    R = np.roll(L, -10, axis=1)
    n = 260
    rng = np.random.default_rng(5)
    xy_l = np.stack([rng.integers(30, W - 8, n), rng.integers(6, H - 6, n)], 1).astype(np.float32)
    # (one left keypoint per right twin and distinct descriptors: each finds its own twin at distance 0)
    d = _desc(n, 6)
    o = np.sort(rng.integers(0, 8, n)).astype(np.int32)
    kl = (xy_l, o, d)
    kr = (xy_l - np.array([10, 0], np.float32), o, d)
    want = _check(ctx, L, R, kl, kr, max_hamming=0, row_tol=0.0)
    print("everything kept: counts3 %s" % (want["counts3"],))
    assert list(want["counts3"]) == [n, n, n]


def test_null_and_hostile_arguments_return_a_status(ctx):
    L, R, kl, kr = _random_scene(7, 10, 10)
    lib, h, p = ctx._lib, ctx._h, _native._p
    m, d = np.zeros(10, np.int32), np.zeros(10, np.float32)
    xy, o, de, kd, xyz, c3 = np.zeros((10, 2), np.float32), np.zeros(10, np.int32), np.zeros((10, 32), np.uint8), np.zeros(10, np.float32), np.zeros((10, 3), np.float32), np.zeros(3, np.int32)
    Qc = np.ascontiguousarray(Q.reshape(16))

    def good():
        return [p(L), p(R), W, H, p(kl[0]), p(kl[1]), p(kl[2]), 10, p(kr[0]), p(kr[1]), p(kr[2]), 10, 4.0, 40.0, 2.0, 75, p(Qc), 7, 3,
                p(m), p(d), p(xy), p(o), p(de), p(kd), p(xyz), p(c3)]
    assert lib.vo_sparse_pair_host(h, *good()) == 0
    assert lib.vo_sparse_pair_host(None, *good()) == VO_E_ARG
    for k in (0, 1, 4, 5, 6, 8, 9, 10, 16, 19, 20, 21, 22, 23, 24, 25, 26):     # every pointer in turn
        a = good()
        a[k] = None
        assert lib.vo_sparse_pair_host(h, *a) == VO_E_ARG, k
    for k, v, code in ((2, 0, VO_E_ARG), (3, -1, VO_E_ARG), (2, 4096, VO_E_CAP), (7, -1, VO_E_ARG), (11, -1, VO_E_ARG), (7, 10 ** 6, VO_E_CAP),
                       (11, 70000, VO_E_CAP), (12, -1.0, VO_E_ARG), (13, 3.0, VO_E_ARG), (13, float("nan"), VO_E_ARG), (13, float("inf"), VO_E_ARG),
                       (14, -0.5, VO_E_ARG), (14, float("nan"), VO_E_ARG), (15, -1, VO_E_ARG), (15, 257, VO_E_ARG)):
        a = good()
        a[k] = v
        assert lib.vo_sparse_pair_host(h, *a) == code, (k, v)
    bad = kl[1].copy()
    bad[3] = 8
    a = good()
    a[5] = p(bad)
    assert lib.vo_sparse_pair_host(h, *a) == VO_E_ARG
    bad = kr[1].copy()
    bad[0] = -1
    a = good()
    a[9] = p(bad)
    assert lib.vo_sparse_pair_host(h, *a) == VO_E_ARG
    # ... and the seam still works
    _check(ctx, L, R, kl, kr)
