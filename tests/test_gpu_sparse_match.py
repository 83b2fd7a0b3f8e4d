"""vo_sparse_match_host (association + sub-pixel refinement of the sparse stereo depth, k_sparse_match) against the numpy
restatement tests/sparse_stereo_ref.py on constructed inputs: match_out equal, disp_out equal as float32 bit patterns.
96 x 64 images, at most 130 keypoints per side; one context for the module."""
import ctypes

import numpy as np
import pytest

import sparse_stereo_ref as S
from openvo_amd import _native

pytestmark = pytest.mark.gpu

H, W = 64, 96
VO_E_ARG, VO_E_CAP = -1, -4
P = dict(min_disp=4, max_disp=40, row_tol=2.0, max_hamming=75)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 128, 96, 16, 100)
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


def _check(ctx, L, R, kl, kr, want_match=None, **over):
    """kl / kr = (xy, octave, desc); -> (match, disp) of the restatement after holding the kernel to them"""
    p = dict(P, **over)
    xy_l, o_l, d_l = (np.asarray(kl[0], np.float32).reshape(-1, 2), np.asarray(kl[1], np.int32), np.asarray(kl[2], np.uint8).reshape(-1, 32))
    xy_r, o_r, d_r = (np.asarray(kr[0], np.float32).reshape(-1, 2), np.asarray(kr[1], np.int32), np.asarray(kr[2], np.uint8).reshape(-1, 32))
    match = S.associate(xy_l, o_l, d_l, xy_r, o_r, d_r, p["min_disp"], p["max_disp"], p["row_tol"], p["max_hamming"])
    disp = S.refine(L, R, xy_l, xy_r, match, p["min_disp"], p["max_disp"])
    gm, gd = ctx.sparse_match_host(L, R, xy_l, o_l, d_l, xy_r, o_r, d_r, **p)
    assert np.array_equal(gm, match), (gm, match)
    assert np.array_equal(gd.view(np.uint32) | (np.isnan(gd) * np.uint32(0x7FFFFFFF)), disp.view(np.uint32) | (np.isnan(disp) * np.uint32(0x7FFFFFFF))), (gd, disp)
    if want_match is not None:
        assert list(match) == list(want_match), (match, want_match)
    return match, disp


def _shifted(seed, d):
    L = _texture(seed)
    return L, np.roll(L, -d, axis=1)


def test_hamming_ties_go_to_the_lower_index(ctx):
    L, R = _shifted(1, 10)
    d = _desc(1, 2)
    near = _flip(d, 20, 1)
    # rights 1 and 2 tie at distance 20 (identical descriptors), right 0 is farther, right 3 is the same descriptor out of range
    kr = ([[40, 30], [41, 31], [39, 29], [70, 30]], [0, 0, 0, 0], np.concatenate([_flip(d, 30, 2), near, near, near]))
    _check(ctx, L, R, ([[50, 30]], [0], d), kr, want_match=[1])
    kr = (kr[0], kr[1], np.concatenate([near, _flip(d, 30, 2), near, near]))
    _check(ctx, L, R, ([[50, 30]], [0], d), kr, want_match=[0])


def test_octave_differences(ctx):
    L, R = _shifted(3, 10)
    d = _desc(5, 4)
    # left keypoint k (octave 3) has ONE candidate by position (its own row), of octave 1 .. 5
    ys = [10, 20, 30, 40, 50]
    kl = ([[50, y] for y in ys], [3] * 5, d)
    kr = ([[40, y] for y in ys], [1, 2, 3, 4, 5], d)
    _check(ctx, L, R, kl, kr, want_match=[-1, 1, 2, 3, -1], row_tol=0.5)
    # unsorted right octaves (not ORB's canonical order): the whole right set is scanned
    perm = [4, 0, 3, 1, 2]
    kr = ([[40, ys[k]] for k in perm], [[1, 2, 3, 4, 5][k] for k in perm], d[perm])
    _check(ctx, L, R, kl, kr, want_match=[-1, 3, 4, 2, -1], row_tol=0.5)
    # the left octave at both ends of the range
    _check(ctx, L, R, ([[50, 30]] * 2, [0, 7], d[:2]), ([[40, 30]] * 4, [0, 1, 6, 7], d[[0, 0, 1, 1]]), want_match=[0, 2])


@pytest.mark.parametrize("octave", [0, 3, 7])
def test_row_offset_at_and_one_ulp_past_the_tolerance(ctx, octave):
    L, R = _shifted(5, 10)
    tol = np.float32(2.0) * S.scales()[octave]
    past = np.nextafter(tol, np.float32(np.inf))
    d = _desc(4, 6)
    # y_i = 0: the float32 difference IS y_j.  Also from y_i = 40 downwards, where the subtraction rounds: the restatement decides.
    y_at, y_past = np.float32(40) - tol, np.float32(40) - past
    kl = ([[50, 0], [50, 0], [50, 40], [50, 40]], [octave] * 4, d)
    kr = ([[40, tol], [40, past], [40, y_at], [40, y_past]], [octave] * 4, d)
    m, _ = _check(ctx, L, R, kl, kr, max_hamming=0)
    assert m[0] == 0 and m[1] == -1
    assert (np.abs(np.float32(40) - y_at) <= tol) == (m[2] == 2) and (np.abs(np.float32(40) - y_past) <= tol) == (m[3] == 3)


def test_d0_exactly_at_the_range_ends(ctx):
    L, R = _shifted(7, 4)
    d = _desc(6, 8)
    up, dn = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), (lambda v: np.nextafter(np.float32(v), np.float32(-np.inf)))
    ys = [8, 16, 24, 32, 40, 48]
    kl = ([[60, ys[0]], [60, ys[1]], [60, ys[2]], [80, ys[3]], [80, ys[4]], [80, ys[5]]], [0] * 6, d)
    # d0 = 4 exactly / just below 4 / just above 4; d0 = 40 exactly / just above / just below
    kr = ([[56, ys[0]], [up(56), ys[1]], [dn(56), ys[2]], [40, ys[3]], [dn(40), ys[4]], [up(40), ys[5]]], [0] * 6, d)
    _check(ctx, L, R, kl, kr, want_match=[0, -1, 2, 3, -1, 5], row_tol=0.0)


def test_distance_at_and_past_max_hamming(ctx):
    L, R = _shifted(9, 10)
    d = _desc(4, 10)
    kl = ([[50, 10], [50, 20], [50, 30], [50, 40]], [0] * 4, d)
    dr = np.concatenate([_flip(d[0:1], 75), _flip(d[1:2], 76), _flip(d[2:3], 0), _flip(d[3:4], 1)])
    kr = ([[40, 10], [40, 20], [40, 30], [40, 40]], [0] * 4, dr)
    _check(ctx, L, R, kl, kr, want_match=[0, -1, 2, 3], row_tol=0.0)
    _check(ctx, L, R, kl, kr, want_match=[-1, -1, 2, -1], row_tol=0.0, max_hamming=0)
    _check(ctx, L, R, kl, kr, want_match=[0, 1, 2, 3], row_tol=0.0, max_hamming=256)


def test_all_zero_and_all_one_descriptors(ctx):
    L, R = _shifted(11, 10)
    z, o = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    kl = ([[50, 20], [50, 40]], [0, 0], np.concatenate([z, o]))
    kr = ([[40, 20], [40, 40], [39, 20], [39, 40]], [0] * 4, np.concatenate([o, z, z, o]))
    _check(ctx, L, R, kl, kr, want_match=[2, 3], row_tol=0.0, max_hamming=255)
    _check(ctx, L, R, kl, kr, want_match=[0, 1], row_tol=0.0, max_hamming=256, max_disp=10.5)    # only the distance-256 ones in range


def test_windows_touching_each_crop_edge(ctx):
    L, R = _shifted(13, 5)
    pts = [(5 + 5, 30), (4 + 5, 30),          # the right strip: xr - 10 = 0 / -1 ... (x_i = xr + 5)
           (20, 5), (20, 4), (20, 58), (20, 59),
           (90, 30), (91, 30)]               # the left window: x0 + 5 = 95 / 96; the right strip of (90, .): xr = 85, xr + 10 = 95
    pts += [(15.5, 30), (14.5, 30.5), (16.5, 5.5), (20, 4.5)]      # halves round to even
    d = _desc(len(pts), 14)
    kl = (pts, [0] * len(pts), d)
    kr = ([[x - 5, y] for x, y in pts], [0] * len(pts), d)
    m, disp = _check(ctx, L, R, kl, kr, row_tol=0.0)
    assert list(m) == list(range(len(pts)))
    ok = ~np.isnan(disp)
    assert not ok[0] and not ok[1]            # xr = 5 and 4: the strip needs xr >= 10
    assert list(ok[2:8]) == [True, False, True, False, True, False]
    _check(ctx, L, R, ([[20, 30]], [0], d[:1]), ([[10, 30]], [0], d[:1]), want_match=[0])       # xr - 10 = 0: inside
    _check(ctx, L, R, ([[19, 30]], [0], d[:1]), ([[9, 30]], [0], d[:1]), want_match=[0])        # xr - 10 = -1: rejected by the refinement


def test_slide_ends_flat_patch_equal_minima_and_range_after_refinement(ctx):
    L = _texture(15)
    d = _desc(1, 16)
    res = {}
    for off in (-5, -4, 0, 4, 5):
        R = np.roll(L, -(10 + off), axis=1)                      # the true match lies `off` columns left of the associated keypoint
        res[off] = _check(ctx, L, R, ([[60, 30]], [0], d), ([[50, 30]], [0], d), want_match=[0])[1][0]
    assert np.isnan(res[-5]) and np.isnan(res[5]) and np.rint(res[-4]) == 6 and np.rint(res[0]) == 10 and np.rint(res[4]) == 14
    # den = 0: a flat patch, and a patch constant along x
    F = np.full((H, W), 77, np.uint8)
    assert np.isnan(_check(ctx, F, F, ([[60, 30]], [0], d), ([[50, 30]], [0], d), want_match=[0])[1][0])
    C = np.repeat(_texture(17)[:, :1], W, axis=1)
    assert np.isnan(_check(ctx, C, C, ([[60, 30]], [0], d), ([[50, 30]], [0], d), want_match=[0])[1][0])
    # two equal minima (SAD = 0 at s = -2 and s = +1): the first
    L2, R2 = _texture(18), _texture(19)
    x0, y0, xr = 50, 30, 40
    p3 = np.tile(L2[y0 - 5:y0 + 6, x0 - 5:x0 - 2], (1, 8))
    L2[y0 - 5:y0 + 6, x0 - 5:x0 + 6] = p3[:, :11]
    R2[y0 - 5:y0 + 6, xr - 7:xr + 7] = p3[:, :14]
    dd = _check(ctx, L2, R2, ([[x0, y0]], [0], d), ([[xr, y0]], [0], d), want_match=[0])[1][0]
    assert np.rint(dd) == 12
    # d0 inside the range, the refined disparity just outside: d0 = 4 = min_disp on a copy shifted by 4, delta of either sign
    L3, R3 = _shifted(20, 4)
    xs = np.arange(30, 82, 4)
    kk = ([[x, 30] for x in xs], [0] * len(xs), _desc(len(xs), 21))
    kr = ([[x - 4, 30] for x in xs], kk[1], kk[2])
    m, disp = _check(ctx, L3, R3, kk, kr, row_tol=0.0)
    free = S.refine(L3, R3, kk[0], kr[0], m, 0, 100)
    assert (m >= 0).all() and (free < 4).any() and (free > 4).any()
    assert np.array_equal(np.isnan(disp), free < 4)
    # ... and at the upper end
    L4, R4 = _shifted(22, 40)
    xs = np.arange(52, 88, 3)
    kk = ([[x, 30] for x in xs], [0] * len(xs), _desc(len(xs), 23))
    kr = ([[x - 40, 30] for x in xs], kk[1], kk[2])
    m, disp = _check(ctx, L4, R4, kk, kr, row_tol=0.0)
    free = S.refine(L4, R4, kk[0], kr[0], m, 0, 100)
    assert (free > 40).any() and np.array_equal(np.isnan(disp), ~(free <= 40))


def _random_scene(seed, nl, nr):
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


def test_every_count_combination(ctx):
    """nl and nr in {0, 1, 63, 64, 65, 129}: waves without a keypoint, one partial wave of candidates, more than one block"""
    sizes, accepted, kept = (0, 1, 63, 64, 65, 129), 0, 0
    for a, nl in enumerate(sizes):
        for b, nr in enumerate(sizes):
            L, R, kl, kr = _random_scene(100 + 10 * a + b, nl, nr)
            m, disp = _check(ctx, L, R, kl, kr)
            accepted += int((m >= 0).sum())
            kept += int((~np.isnan(disp)).sum())
    print("accepted %d, kept %d over the 36 combinations" % (accepted, kept))
    assert accepted >= 100 and kept >= 30


def test_hostile_arguments_return_a_status(ctx):
    L, R, kl, kr = _random_scene(7, 10, 10)
    lib, h, p = ctx._lib, ctx._h, _native._p
    m, d = np.zeros(10, np.int32), np.zeros(10, np.float32)
    good = [p(L), p(R), W, H, p(kl[0]), p(kl[1]), p(kl[2]), 10, p(kr[0]), p(kr[1]), p(kr[2]), 10, 4.0, 40.0, 2.0, 75, p(m), p(d)]
    assert lib.vo_sparse_match_host(h, *good) == 0
    for k in (0, 1, 4, 5, 6, 8, 9, 10, 16, 17):                  # every pointer in turn
        bad = list(good)
        bad[k] = None
        assert lib.vo_sparse_match_host(h, *bad) == VO_E_ARG, k
    assert lib.vo_sparse_match_host(None, *good) == VO_E_ARG
    for k, v in ((2, -1), (3, 0), (7, -1), (11, -5), (15, -1), (15, 257), (12, -1.0), (13, 4.0), (13, 3.0), (14, -0.5)):
        bad = list(good)
        bad[k] = v
        assert lib.vo_sparse_match_host(h, *bad) == VO_E_ARG, (k, v)
    for k in (12, 13, 14):
        for v in (float("nan"), float("inf")):
            if (k, v) == (12, float("inf")):
                continue
            bad = list(good)
            bad[k] = v
            assert lib.vo_sparse_match_host(h, *bad) == VO_E_ARG, (k, v)
    bad = list(good)
    bad[12] = float("inf")
    assert lib.vo_sparse_match_host(h, *bad) == VO_E_ARG
    big = (np.zeros((70000, 2), np.float32), np.zeros(70000, np.int32), np.zeros((70000, 32), np.uint8))
    bad = list(good)
    bad[8:12] = [p(big[0]), p(big[1]), p(big[2]), 70000]
    assert lib.vo_sparse_match_host(h, *bad) == VO_E_CAP
    bad = list(good)
    bad[2], bad[3] = 4096, 4096
    assert lib.vo_sparse_match_host(h, *bad) == VO_E_CAP
    o_bad = np.array(kl[1], np.int32)
    o_bad[3] = 8
    bad = list(good)
    bad[5] = p(o_bad)
    assert lib.vo_sparse_match_host(h, *bad) == VO_E_ARG
    # sparse_stereo / download_keypoint_depth: the same care
    c3 = np.zeros(3, np.int32)
    assert lib.vo_sparse_stereo(h, 0, 50, 4.0, 40.0, 2.0, 75, None) == VO_E_ARG
    assert lib.vo_sparse_stereo(h, -1, 50, 4.0, 40.0, 2.0, 75, p(c3)) == VO_E_ARG
    assert lib.vo_sparse_stereo(h, 0, 50, float("nan"), 40.0, 2.0, 75, p(c3)) == VO_E_ARG
    assert lib.vo_sparse_stereo(h, 0, 50, 4.0, 40.0, 2.0, 75, p(c3)) == -3            # no pair in the slot
    assert lib.vo_download_keypoint_depth(h, 0, None, None, 0, None) == -3
    assert lib.vo_download_keypoint_depth(h, 99, None, None, 0, None) == VO_E_ARG
    # the context still works
    _check(ctx, L, R, kl, kr)


def test_misuse_sweep_over_the_three_entries():
    """The sweep of tests/abi_misuse.py for the sparse entries, on a fresh context (nothing configured): a NULL context, every
    pointer NULL, hostile integers and floats -- a status every time, and success never."""
    fresh = _native.Context(0, 320, 240, 64, 200)
    lib = fresh._lib
    ints = [-1, 0, 1, 27, 28, 1000, 2**31 - 1, -2**31]
    rng = np.random.default_rng(5)
    calls = 0
    try:
        for name in ("vo_sparse_stereo", "vo_download_keypoint_depth", "vo_sparse_match_host"):
            f = getattr(lib, name)
            for variant in range(8):
                args = []
                for k, t in enumerate(f.argtypes):
                    if k == 0:
                        args.append(None if variant == 0 else fresh._h)
                    elif t is ctypes.c_int:
                        args.append(int(rng.choice(ints)) if variant > 1 else (0 if variant == 0 else -1))
                    elif t is ctypes.c_float:
                        args.append(float(rng.choice([0.0, -1.0, 0.8, float("nan"), 1e30])))
                    else:
                        args.append(None)
                rc = f(*args)
                calls += 1
                assert rc in (-1, -3, -4), (name, variant, args[1:], rc)
    finally:
        fresh.close()
    assert calls == 24
