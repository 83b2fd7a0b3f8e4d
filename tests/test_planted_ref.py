"""The references of the planted-slot tests (tests/planted.py) against each other, on the CPU: the numpy fit against the
kernel-order restatement (tests/pose_fit_ref.py, n <= 1024) and the CPU oracle's Umeyama (any n), the numpy brute-force matcher
against the oracle's kNN-2 + ratio filter, on every geometry builder and every size the GPU tests use.  And the seam itself: only
the test-only build of the library exports the planting entry.

Bound of the fit comparisons: 1e-11 per element of T.  Two double-precision evaluations of one well-conditioned fit (s2 / s1 of
the covariance above 1e-6, asserted) differ by rounding in sums of up to 2000 terms of magnitude <= 80^2, i.e. some 1e-13
(measured over n = 3 .. 1024 and all builders: at most 4.3e-13, x8 coordinates at n = 3); 1e-11 leaves that its room and stays two
orders inside the 1e-9 the GPU tests hold the fused step to against the same numpy fit."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted as P                        # noqa: E402
import pose_fit_ref as PF                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (3, 4, 9, 10, 11, 64, 65, 127, 128, 129, 512, 513, 1024, 1025, 2000)
NUMERIC = [g for g in sorted(P.GEOMETRY) if g not in P.RANK_DEFICIENT + P.SPECIAL]
BOUND = 1e-11


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build_oracle()
    return O


@pytest.mark.parametrize("geom", NUMERIC)
def test_numpy_fit_agrees_with_the_restatement_and_the_oracle(oracle, geom):
    worst = 0.0
    for n in SIZES:
        if geom == "dup" and n < 6:
            continue                      # (every pair twice: two distinct points, a rank-deficient set -- see below)
        pa, pb = P.geometry(geom, n)
        T, rc, cond = P.np_fit(pa, pb)
        assert rc == 0 and cond > 1e-6, (geom, n, rc, cond)
        To, _ = oracle.umeyama(pa, pb)
        d = float(np.abs(T - To).max())
        if n <= 1024:
            Tr, _, rcr = PF.umeyama(pa, pb)
            assert rcr == 0
            d = max(d, float(np.abs(T - Tr).max()))
        worst = max(worst, d)
        assert d <= BOUND, (geom, n, d)
        assert abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-9, (geom, n)           # a rotation, also for the mirrored target
    print("%s: largest |T numpy - T restated / oracle| = %.3g" % (geom, worst))


@pytest.mark.parametrize("geom", P.RANK_DEFICIENT)
def test_rank_deficient_sets_are_refused_by_every_reference(oracle, geom):
    for n in (3, 10, 64, 1024, 1025):
        pa, pb = P.geometry(geom, n)
        assert P.np_fit(pa, pb)[1] == -2
        if n <= 1024:
            assert PF.umeyama(pa, pb)[2] == -2
        with pytest.raises(ValueError, match="colinear"):
            oracle.umeyama(pa, pb)


def test_two_distinct_points_are_ill_conditioned_for_every_reference():
    """two distinct points, each twice: rank one up to rounding.  The references return a status of 0 and transforms that need not
    agree (numpy against the Jacobi restatement: 0.48); such a set is compared through rc and bit for bit with the restatement"""
    pa, pb = P.geometry("dup", 4)
    T, rc, cond = P.np_fit(pa, pb)
    assert rc == 0 and cond < 1e-6
    assert PF.umeyama(pa, pb)[2] == 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_fewer_than_three_points_and_non_finite_points():
    pa, pb = P.geometry("rigid", 2)
    assert P.np_fit(pa, pb)[1] == -1 and PF.umeyama(pa, pb)[2] == -1
    pa, pb = P.geometry("nonfinite", 64)
    T, rc, _ = P.np_fit(pa, pb)
    Tr, _, rcr = PF.umeyama(pa, pb)
    assert rc == 0 and rcr == 0 and np.isnan(T).all() and np.isnan(Tr).all()
    f = P.np_pose_fit(pa, pb)
    assert (f["n2"], f["rc1"], f["rc2"], f["nan"]) == (0, 0, 1, 1)
    r = P.restated(pa, pb)
    assert (r["n2"], r["rc1"], r["rc2"]) == (0, 0, 1)


@pytest.mark.parametrize("geom", ["soft", "dup", "mirrored", "rigid_out"])
def test_numpy_outlier_rule_agrees_with_the_restatement(geom):
    """first fit, np.median threshold, kept set and final fit: the same n2 and status, T1 / T2 within the bound"""
    for n in (9, 10, 11, 14, 64, 65, 127, 128, 129, 512, 513, 1024):
        pa, pb = P.geometry(geom, n)
        for mm in (9, 10, 11):
            f, r = P.np_pose_fit(pa, pb, P.OUTLIER, mm), P.restated(pa, pb, P.OUTLIER, mm)
            assert (f["n2"], f["rc1"], f["rc2"]) == (r["n2"], r["rc1"], r["rc2"]), (geom, n, mm)
            assert f["cond"] > 1e-6 and f["gap"] > 1e-9, (geom, n, f["cond"], f["gap"])
            for k in ("T1", "T2"):
                assert (f[k] is None) == (r[k] is None), (geom, n, mm, k)
                if f[k] is not None:
                    assert np.abs(f[k] - r[k]).max() <= BOUND, (geom, n, mm, k)
        if n >= 10:
            assert f["n2"] < n, (geom, n)              # (the pass had something to remove)


def _tied_descriptors(n, rng):
    """descriptors that differ in their first byte only: distances 0 .. 8, ties everywhere"""
    d = np.zeros((n, 32), np.uint8)
    d[:, 0] = rng.integers(0, 256, n)
    return d


def test_numpy_matcher_equals_the_oracle(oracle):
    rng = np.random.default_rng(5)
    sets = [P.descriptors(nq, M, rng)[:2] for nq, M in ((3600, 40), (512, 512), (513, 512), (5, 0), (2, 2), (64, 1))]
    sets += [(_tied_descriptors(300, rng), _tied_descriptors(40, rng)), (_tied_descriptors(7, rng), _tied_descriptors(2, rng))]
    for dq, dt in sets:
        idx, dist = P.knn2(dq, dt)
        oi, od = oracle.bf_knn2_hamming(dq, dt)
        assert np.array_equal(idx, oi) and np.array_equal(dist, od)
        for ratio in (0.8, 0.5, 1.0):
            q, t = P.ratio_test(idx, dist, ratio)
            oq, ot = oracle.ratio_filter(oi, od, ratio)
            assert np.array_equal(q, oq) and np.array_equal(t, ot)


def test_a_case_meets_its_match_count(oracle):
    for nq, M in ((3600, 40), (64, 64), (5, 0), (600, 600)):
        c = P.Case("c", nq, M).build()
        m = c.model(oracle)
        assert m["counts"][0] == M and len(m["q"]) == M
        assert np.array_equal(m["pa"], c.xyz_a[m["q"]]) and m["counts"][1] == int(m["keep"].sum())


def test_threshold_builder_sits_on_the_threshold(oracle):
    """the five positions: consistent exactly when the float32 difference is BELOW the float32 threshold"""
    pa, pb = P.geometry("threshold", 10)
    x = pb[:, 0]
    d = np.abs(x[:, None] - x[None, :])
    assert (d == P.THR32).any() and (d == np.nextafter(P.THR32, np.float32(0))).any() and (d == np.nextafter(P.THR32, np.float32(1))).any()
    want = (d < P.THR32).sum(0)
    seed = int(np.argmax(want))
    mask = oracle.rigid_clique(pa, pb, P.RIGIDITY)
    assert mask[seed] == 1 and all(d[i, j] < P.THR32 for i in np.nonzero(mask)[0] for j in np.nonzero(mask)[0])


def test_only_the_test_build_exports_the_planting_entry():
    """the product library has no way to plant keypoints (next to: it has no failure injection)"""
    prod = os.path.join(ROOT, "openvo_amd", "libvo355.so")
    hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
    assert os.path.exists(prod) and os.path.exists(hooks), "build the libraries first (__graft_entry__.build())"
    for entry in ("vo_test_plant_keypoints", "vo_test_plant_dense"):
        assert not hasattr(ctypes.CDLL(prod), entry), entry
        assert hasattr(ctypes.CDLL(hooks), entry), entry
