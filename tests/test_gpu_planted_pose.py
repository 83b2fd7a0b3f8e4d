"""The fused pose step (k_pose_prep -> k_pose_cons_bits -> k_pose_solve, csrc/geom.hip) driven on purpose through every clique and
fit regime: keypoints, descriptors and 3-D points are PLANTED in two slots (vo_test_plant_keypoints of the test-only library), so
(nq, M) and the geometry are chosen, not what ORB finds in the corridor.  References: tests/planted.py -- numpy brute-force
matches, oracle.rigid_clique, a high-precision numpy fit with the np.median outlier rule -- and, up to 1024 pairs, the kernel-order
restatement tests/pose_fit_ref.py bit for bit.

Every case, through pose_pair AND pose_pair_begin / _end (equal records):
    counts4 = (M, n1, n2, flags) and rc2 exact; q / t of point_clouds exact, pa / pb as bit patterns of xyz[q] / xyz[t];
    T1 / T2 within 1e-9 of the numpy fit (only where the reference's own s2 / s1 > 1e-6: asserted, never skipped);
    n1 <= 1024: T1 / T2 np.array_equal with the restatement;   n1 > 1024: no reference residual within 1e-9 of the threshold.

Boundaries, from pose_enqueue / pose_check / k_pose_solve (m_cap = nq rounded up to even, words = ceil(nq / 64)):
    nq <= 512                       consistency rows computed inside k_pose_solve (cons_inline), register-resident clique
    nq >= 513                       k_pose_cons_bits; M <= 512 and bits_cap >= 64 M: lane bytes + register-resident clique
    clique_fast<2 | 4 | 8>          M <= 128 | 256 | 512
    16 m_cap + 8 nq words <= 56 KB  bit matrix in LDS: nq <= 597 (598: rows read from HBM, bits_cap = 0)
    16 m_cap > 56 KB                nq >= 3585: the four set arrays in the global workspace (sets_global)
    16 nq > 60 KB                   nq >= 3841: VO_E_CAP
    n1 < 10                         no first fit;  n1 <= 512: ranks in LDS (parts = min(1024 / n1, 8): 8 up to 128, 7 .. 2 up to 512);
    n1 > 512                        ranks from the global residuals;  n <= 1024: one-wave sums;  n > 1024: block sums

Non-finite coordinates.  Read before these cases ran on a GPU: a row with an inf / NaN coordinate compares false everywhere
(diagonal included), so its count is 0 and it is a candidate of nothing.  The three clique paths take every index from the low
16 bits of a wave maximum over keys ((count + m) << 16 | 0xFFFF - j) built for j < m only, with a key above zero for every such j
(count >= -count * 1 + m >= 0): seed and sel lie in [0, m).  Each greedy loop runs `it < m` whatever the sums are (a negative
candidate sum, reached when the seed row itself is non-finite, only keeps it running to that bound).  The fit skips the rank
pass on a NaN residual, its compaction keeps nothing (x < NaN is false), dev_svd3 ends after 60 sweeps.

One child process per group of cases, VO355_LIB pointing at the test-only library; the cases are the parametrisation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted as P                        # noqa: E402
from planted import Case                   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_STATE, VO_E_CAP = -3, -4
BAR = 1e-9                                 # the bar every fused pose of this project is held to
NOF = dict(rigidity=0.0)                   # the clique filter off: n1 = M

GROUPS = {
    # nq decides where the consistency rows and the sets live
    "nq": [
        Case("nq2_M2_inline", 2, 2, "rigid", min_matches=1),
        Case("nq64_M40_inline", 64, 40),
        Case("nq512_M512_inline_fast8", 512, 512),
        Case("nq513_M512_consbits_lanebytes_fast8", 513, 512),
        Case("nq513_M513_generic_lds_bits", 513, 513),
        Case("nq597_M597_largest_lds_bits", 597, 597),
        Case("nq598_M598_hbm_bits", 598, 598),
        Case("nq598_M40_hbm_bits", 598, 40),
        Case("nq3584_M40_lds_sets", 3584, 40),
        Case("nq3585_M40_sets_global", 3585, 40),
        Case("nq3600_M40", 3600, 40),
        Case("nq3584_M3584_lds_sets", 3584, 3584, "rigid_sparse150"),
        Case("nq3840_M3840_sets_global", 3840, 3840, "rigid_sparse150"),
        Case("nq513_M513_filter_off", 513, 513, "soft", **NOF),
        Case("nq3585_M40_filter_off", 3585, 40, "soft", **NOF),
    ],
    # M decides the clique path (nq = M + 3 up to 512: inline rows)
    "clique": [Case("M%d" % M, min(M + 3, 512), M, "rigid" if M < 64 else "rigid_out", min_matches=(1 if M < 10 else 10)) for M in (0, 1, 2, 3, 9, 10, 11, 64, 65, 128, 129, 256, 257, 511, 512)] + [
        Case("M0_min_matches_0", 5, 0, min_matches=0),
        Case("tie_two_groups_fast", 64, 64, "two_groups"),
        Case("tie_two_groups_fast4_odd", 201, 201, "two_groups"),
        Case("at_threshold_fast", 64, 64, "threshold"),
        Case("clique_of_one_fast", 64, 64, "clique_one"),
        Case("tie_two_groups_generic_lds", 520, 520, "two_groups"),
        Case("at_threshold_generic_lds", 520, 520, "threshold"),
        Case("clique_of_one_generic_lds", 520, 520, "clique_one"),
        Case("tie_two_groups_generic_hbm", 600, 600, "two_groups"),
        Case("at_threshold_generic_hbm", 600, 600, "threshold"),
        Case("clique_of_one_generic_hbm", 600, 600, "clique_one"),
        Case("at_threshold_sets_global", 3585, 150, "threshold"),
    ],
    # n1 decides the fit path (filter off: n1 = M = nq)
    "fit": [Case("n1_%d_outlier_on" % n, n, n, "soft", **NOF) for n in (9, 10, 11, 127, 128, 129, 512, 513, 1024, 1025, 2000)] +
           [Case("n1_%d_outlier_off" % n, n, n, "soft", outlier=0.0, **NOF) for n in (9, 10, 129, 1024, 1025)] +
           [Case("dup_%s_%d" % ("even" if n % 2 == 0 else "odd", n), n, n, "dup", **NOF) for n in (64, 65, 512, 513, 1025, 1026)] +
           [Case("n2_10_min_matches_%d" % mm, 14, 14, "soft14", min_matches=mm, **NOF) for mm in (9, 10, 11)],
    # every geometry builder through the whole step, one-wave and block sums
    "geometry64": [Case("%s_64" % g, 67, 64, g) for g in P.ALL_BUILDERS],
    "geometry1025": [Case("%s_1025" % g, 1030, 1025, g) for g in P.ALL_BUILDERS if g not in ("threshold", "nonfinite")] +
                    [Case("threshold_1025_filter_off", 1025, 1025, "threshold", **NOF)],
    "nonfinite": [
        Case("nonfinite_filter_off_64", 64, 64, "nonfinite", **NOF),
        Case("nonfinite_filter_off_1025", 1025, 1025, "nonfinite", **NOF),
        Case("nonfinite_filter_off_no_first_fit", 9, 9, "nonfinite", min_matches=3, **NOF),
        Case("nonfinite_fast", 64, 64, "nonfinite"),
        Case("nonfinite_fast8_consbits", 513, 400, "nonfinite"),
        Case("nonfinite_generic_lds", 520, 520, "nonfinite"),
        Case("nonfinite_generic_hbm", 1030, 1025, "nonfinite"),
        Case("nonfinite_sets_global", 3585, 40, "nonfinite"),
        Case("all_nonfinite_fast", 12, 12, "all_nonfinite"),
        Case("all_nonfinite_generic", 520, 520, "all_nonfinite"),
    ],
}


ALL_CASES = [(g, c.name) for g in GROUPS for c in GROUPS[g]]


# ------------------------------------------------------------------------------------------------ in the child process
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_T(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _plant(ctx, c, sa=0, sb=1):
    ctx.plant_keypoints(sa, c.xy_a, c.dq, c.xyz_a)
    ctx.plant_keypoints(sb, c.xy_b, c.dt, c.xyz_b)


def _check_case(ctx, O, c):
    """plant, run the step both ways, hold it to the references -> the figures of the case"""
    c.build()
    m = c.model(O)
    _plant(ctx, c)
    q, t, pa, pb, sa, sb = ctx.point_clouds(0, 1, P.RATIO)
    assert np.array_equal(q, m["q"]) and np.array_equal(t, m["t"]), "matches differ from the numpy brute force"
    assert np.array_equal(_bits(pa), _bits(m["pa"])) and np.array_equal(_bits(pb), _bits(m["pb"])) and not sa.any() and not sb.any()
    args = (0, 1, P.RATIO, c.min_matches, c.rigidity, c.outlier)
    counts, rc, T1, T2 = ctx.pose_pair(*args)
    counts_b, rc_b, T1_b, T2_b = ctx.pose_pair_end(ctx.pose_pair_begin(*args))
    fig = dict(nq=c.nq, M=int(counts[0]), n1=int(counts[1]), n2=int(counts[2]), flags=int(counts[3]), rc=[int(rc[0]), int(rc[1])], dT=0.0)
    print("%s: (nq, M, n1, n2) = (%d, %d, %d, %d) flags %d rc %s, want counts %s rc %s" % (c.name, c.nq, *counts[:3], counts[3], rc, m["counts"], m["rc"]), flush=True)
    assert np.array_equal(counts, counts_b) and np.array_equal(rc, rc_b), "pose_pair and pose_pair_begin / _end differ"
    assert tuple(counts) == m["counts"], "counts4 %s, want %s" % (counts, m["counts"])
    assert tuple(rc) == m["rc"], "rc2 %s, want %s" % (rc, m["rc"])
    n1 = m["counts"][1]
    r = P.restated(m["qa"], m["qb"], c.outlier, c.min_matches) if n1 <= 1024 else None
    if r is not None:
        assert (r["n2"], r["rc1"], r["rc2"]) == (m["counts"][2], *m["rc"]), "the restatement and the numpy fit disagree: %s" % (r,)
    else:
        assert m["gap"] > 1e-9, "a reference residual lies within 1e-9 of the threshold (%.3g): choose other inputs" % m["gap"]
    for k, got, got_b, code in (("T1", T1, T1_b, rc[0]), ("T2", T2, T2_b, rc[1])):
        if code != 0:
            continue
        assert _same_T(got, got_b), "%s: pose_pair and pose_pair_begin / _end differ" % k
        want = m[k]
        if np.isnan(want).any():
            assert np.isnan(want).all() and np.isnan(got).all(), "%s: a non-finite input must give a NaN transform" % k
        else:
            assert m["cond"] > 1e-6, "%s: the reference itself is ill-conditioned here (s2 / s1 = %.3g)" % (k, m["cond"])
            d = float(np.abs(got - want).max())
            fig["dT"] = max(fig["dT"], d)
            print("    %s: |T - numpy| = %.3g" % (k, d), flush=True)
            assert d <= BAR, "%s differs from the numpy fit by %.3g" % (k, d)
        if r is not None:
            assert _same_T(got, r[k]), "%s is not bit-identical with the kernel-order restatement (max diff %.3g)" % (k, float(np.nanmax(np.abs(got - r[k]))))
    return fig


def _small_context():
    from openvo_amd import _native
    ctx = _native.Context(0, 64, 64, 16, 4096)        # image size is irrelevant; kp_cap = 9216 > 3840
    Q = np.eye(4)
    Q[3, 3] = 0.0; Q[2, 3] = 50.0; Q[3, 2] = 10.0
    ctx.set_Q(Q)
    return ctx


def _run_cases(ctx, O, cases, check=_check_case):
    out = {}
    for c in cases:
        try:
            out[c.name] = dict(ok=True, **check(ctx, O, c))
        except AssertionError as e:                    # (anything else -- a native error status, a fault -- ends the child)
            out[c.name] = dict(ok=False, err=str(e)[:1500])
            print("%s: FAILED %s" % (c.name, out[c.name]["err"]), flush=True)
    return out


def _group_body(group):
    from oracle import oracle as O
    ctx = _small_context()
    out = _run_cases(ctx, O, GROUPS[group])
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _cap_body():
    """3841 query keypoints: VO_E_CAP from both entries, and the step after it is exact"""
    from openvo_amd import _native
    from oracle import oracle as O
    ctx = _small_context()
    big = Case("nq3841", 3841, 40).build()
    _plant(ctx, big)
    for call in (lambda: ctx.pose_pair(0, 1, P.RATIO, 10, P.RIGIDITY, P.OUTLIER), lambda: ctx.pose_pair_begin(0, 1, P.RATIO, 10, P.RIGIDITY, P.OUTLIER)):
        with pytest.raises(_native.VoError) as e:
            call()
        assert e.value.code == VO_E_CAP, e.value
    q, t = ctx.point_clouds(0, 1, P.RATIO)[:2]         # (the composed path has no such bound)
    assert len(q) == 40
    out = _run_cases(ctx, O, [Case("after_the_refusal_nq3840_M40", 3840, 40), Case("after_the_refusal_nq64", 64, 50)])
    ctx.close()
    assert all(v["ok"] for v in out.values()), out
    print("PLANTED-RESULT " + json.dumps(out))


def _plant_refusals_body():
    from openvo_amd import _native
    ctx = _small_context()
    c = Case("c", 8, 4).build()
    for bad in (lambda: ctx.plant_keypoints(-1, c.xy_a, c.dq, c.xyz_a), lambda: ctx.plant_keypoints(_native.VO_NUM_SLOTS, c.xy_a, c.dq, c.xyz_a)):
        with pytest.raises(_native.VoError) as e:
            bad()
        assert e.value.code == -1
    n = ctx.kp_cap + 1
    with pytest.raises(_native.VoError) as e:
        ctx.plant_keypoints(0, np.zeros((n, 2), np.float32), np.zeros((n, 32), np.uint8), np.zeros((n, 3), np.float32))
    assert e.value.code == VO_E_CAP
    lib, vp = ctx._lib, __import__("ctypes").c_void_p
    assert lib.vo_test_plant_keypoints(ctx._h, 0, 4, None, None, None, None) == -1
    assert lib.vo_test_plant_keypoints(ctx._h, 0, 4, vp(c.xy_a.ctypes.data), vp(c.dq.ctypes.data), None, None) == -1
    with pytest.raises(_native.VoError) as e:          # nothing was planted: the slot holds no keypoints
        ctx.pose_pair(0, 1, P.RATIO, 10, 0, 0)
    assert e.value.code == VO_E_STATE
    ctx.close()
    print("PLANTED-RESULT {}")


def _pnp_body():
    """pnp_pair on planted slots: usable n in {0, 3, 4, 5} with non-finite 3-D points interleaved"""
    ctx = _small_context()
    K4 = [50.0, 50.0, 32.0, 32.0]
    ITERS, THR, SEED = 64, 1.5, 4321
    out = {}
    for n_use in (0, 3, 4, 5):
        M = 2 * n_use + 3
        c = Case("pnp_n%d" % n_use, M + 5, M, "rigid").build()
        q, t = P.matches(c.dq, c.dt)
        assert len(q) == M
        bad = np.ones(M, bool)
        bad[1:2 * n_use:2] = False                     # usable: match 1, 3, 5, ...
        c.xyz_a[q[bad], np.arange(int(bad.sum())) % 3] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf][:int(bad.sum())]
        X = c.xyz_a[q]
        ok = np.isfinite(X).all(1)
        assert int(ok.sum()) == n_use
        c.xy_b[t[ok]] = (X[ok, :2] / X[ok, 2:3] * 50.0 + 32.0).astype(np.float32)      # slot b sees the points where they are
        _plant(ctx, c)
        uv = c.xy_b[t[ok]]
        r = ctx.pnp_pair(0, 1, P.RATIO, K4, ITERS, THR, SEED, want_matches=True)
        tk = ctx.pnp_pair_begin(0, 1, P.RATIO, K4, ITERS, THR, SEED, want_matches=True)
        r2 = ctx.pnp_pair_end(tk, want_matches=True)
        print("%s: hdr (M, n, flags) = (%d, %d, %d), best_count %d" % (c.name, r["matches"], r["n"], r["flags"], r["best_count"]), flush=True)
        for k in ("matches", "n", "flags", "best_iter", "best_count"):
            assert r[k] == r2[k], k
        for k in ("Rt", "mask", "q", "t"):
            assert np.array_equal(r[k], r2[k]), k
        assert (r["matches"], r["n"], r["flags"]) == (M, n_use, 0)
        assert np.array_equal(r["q"], q[ok]) and np.array_equal(r["t"], t[ok])
        if n_use >= 4:
            ref = ctx.ransac_pnp(X[ok], uv, K4, ITERS, THR, SEED)
            assert (r["best_iter"], r["best_count"]) == (ref["best_iter"], ref["best_count"]) and ref["best_count"] == n_use
            assert np.array_equal(r["Rt"], ref["Rt"]) and np.array_equal(r["mask"], ref["mask"])
        else:
            assert r["best_count"] == 0 and not r["mask"].any()       # fewer than 4: no pose, no inlier
        out[c.name] = dict(ok=True, M=M, n=n_use)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _slot_body():
    """what a planted slot holds, what clears it, and that real slots beside it are untouched"""
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    from oracle import oracle as O
    ctx = _native.Context(0, 640, 480, 64, 500)
    cor = Corridor("C1")
    cam = StereoCamera(cor.K(), cor.dist(), cor.K(), cor.dist(), cor.rect_params(), cor.sgbm_params(), (cor.w, cor.h), context=ctx)
    pairs = cor.pairs(0, 2)
    for s, (L, R) in zip((12, 13), pairs):             # a plain dense C1 pair
        ctx.upload_pair(s, L, R, True)
        ctx.sgbm_compute(s)
        ctx.orb_slot_count(s, 500, 0)
    real = ctx.pose_pair(12, 13, P.RATIO, 10, P.RIGIDITY, P.OUTLIER)
    assert real[0][2] >= 10 and real[1][1] == 0
    ctx.upload_pair(1, *pairs[0], True)                # slot 1 holds an image pair under the planted keypoints
    c = Case("slot_64", 64, 50)
    fig = _check_case(ctx, O, c)
    assert fig["M"] == 50
    rd = np.random.default_rng(3).integers(0, 256, (len(c.dt), 32), dtype=np.uint8)
    ctx.plant_keypoints(1, c.xy_b, c.dt, c.xyz_b, rd)
    for s, xy, desc, xyz, rdesc in ((0, c.xy_a, c.dq, c.xyz_a, np.zeros_like(c.dq)), (1, c.xy_b, c.dt, c.xyz_b, rd)):
        k = ctx.download_keypoints(s)
        assert np.array_equal(k["xy"], xy) and np.array_equal(k["desc"], desc)
        for name in ("size", "angle", "response", "octave"):
            assert len(k[name]) == len(xy) and not k[name].any(), name
        got_xyz, got_disp = ctx.download_keypoint_depth(s)
        assert np.array_equal(_bits(got_xyz), _bits(xyz)) and len(got_disp) == len(xy) and not got_disp.any()
        assert np.array_equal(ctx.download_keypoint_rdesc(s), rdesc)
    again = ctx.pose_pair(12, 13, P.RATIO, 10, P.RIGIDITY, P.OUTLIER)
    for a, b in zip(real, again):
        assert np.array_equal(a, b), "planting changed the pose of two real slots"
    # sparse_stereo into the planted slot replaces what was planted, as it replaces any sparse result
    params = (4, 100, 2.0, 75)
    ctx.upload_pair(2, *pairs[0], True)
    want3, got3 = ctx.sparse_stereo(2, 500, *params), ctx.sparse_stereo(1, 500, *params)
    assert np.array_equal(want3, got3) and got3[2] >= 200
    for a, b in zip(ctx.download_keypoint_depth(2), ctx.download_keypoint_depth(1)):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(ctx.download_keypoints(2)["desc"], ctx.download_keypoints(1)["desc"])
    # an upload into the planted slot clears it
    ctx.upload_pair(0, *pairs[1], True)
    for call in (lambda: ctx.pose_pair(0, 1, P.RATIO, 10, 0, 0), lambda: ctx.download_keypoint_depth(0)):
        with pytest.raises(_native.VoError) as e:
            call()
        assert e.value.code == VO_E_STATE
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(dict(slot=dict(ok=True, **fig))))


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    """run tests.test_gpu_planted_pose.<body> once in a process of its own against the test-only library -> its result dict"""
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_planted_pose as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANTED-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("PLANTED-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("PLANTED-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("group,name", ALL_CASES, ids=["%s-%s" % gc for gc in ALL_CASES])
def test_planted_regime(group, name):
    res = _child("_group_body(%r)" % group)[name]
    assert res["ok"], res["err"]
    print("%s: (nq, M, n1, n2) = (%d, %d, %d, %d), largest |T - numpy| = %.3g" % (name, res["nq"], res["M"], res["n1"], res["n2"], res["dT"]))


def test_the_regimes_reach_what_they_name():
    """the (n1, n2) a case reaches are what its name promises: the fit cases keep n2 below n1, the sparse sets a clique of 150"""
    for c in GROUPS["fit"]:
        res = _child("_group_body('fit')")[c.name]
        assert res["n1"] == c.nq
        if c.outlier > 0 and c.nq >= 10:
            assert res["n2"] < res["n1"], c.name
    res = _child("_group_body('fit')")
    assert [res["n2_10_min_matches_%d" % mm]["rc"][1] for mm in (9, 10, 11)] == [0, 0, 1] and res["n2_10_min_matches_10"]["n2"] == 10
    res = _child("_group_body('nq')")
    assert res["nq3840_M3840_sets_global"]["n1"] >= 150 and res["nq3584_M3584_lds_sets"]["n1"] >= 150


def test_more_than_3840_query_keypoints_are_refused_and_the_next_step_is_exact():
    _child("_cap_body()")


def test_planting_refuses_bad_arguments():
    _child("_plant_refusals_body()")


def test_pnp_pair_on_planted_slots():
    _child("_pnp_body()")


def test_a_planted_slot_is_a_sparse_slot_like_any_other():
    _child("_slot_body()")
