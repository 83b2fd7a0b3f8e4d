"""The fused PnP step (vo_pnp_pair: k_pnp_prep in csrc/geom.hip -> k_pnp_hyp -> k_pnp_score -> k_pnp_finish in csrc/ransac.hip) driven on
purpose through every regime of its loops: keypoints, descriptors, 3-D points and right descriptors are PLANTED in two slots
(vo_test_plant_keypoints of the test-only library), so (nq, M), the unusable matches, the inliers and their places are chosen,
not what ORB finds in the corridor.  The inputs and the model are tests/planted_pnp.py; tests/test_planted_pnp_ref.py asserts,
without a GPU, that every case reaches the regime its name promises.

Every case, through pnp_pair(..., want_matches=True) AND pnp_pair_begin / _end (equal in every field, the tails of the arrays included):
    matches, n, flags exact; q, t exact against the numpy matches and the finite filter in match order
    mask[:n] exact against oracle.ransac_pnp;  mask[n:nq] == 0;  q[n:nq] == t[n:nq] == -1
    best_iter, best_count exact;  Rt within 1e-10 of the oracle and bit-identical with ctx.ransac_pnp on the model's compacted arrays
    refine_status, refine_steps exact;  Rt_refined within 1e-9 of the float64 restatement AND of the same refit with np.longdouble
    sums (the project's bar for a pose through reordered float64 sums);  status 1: Rt_refined == Rt

Boundaries, from k_pnp_prep / k_pnp_score / k_pnp_finish (one block of 256 threads = 4 waves each, but k_pnp_score: one wave per hypothesis):
    M <= 256                        one pass of k_pnp_prep's second loop: the running count n is only ever 0
    M >= 257                        further passes: a pass's offset is n plus the earlier waves' counts; a whole pass (or wave) may keep nothing
    n < 4                           no pose: all-zero hypotheses, best (0, 0), mask 0
    n <= 64 | 65 ..                 one | several strides of a scoring wave;  iters % 4, iters % 64: the tails of the score / hyp grids
    iters <= 256                    one hypothesis per thread of the winner search;  iters >= 257: h = thread + 256 k, then the shuffle
                                    and the four waves in LDS -- "most inliers, then lowest index" across threads, waves and passes
    best_count 5 | 6                refit not attempted (status 1) | attempted
    n <= 256                        every thread of the refit holds at most one point;  n >= 257: the strided sums, then the DPP tree,
                                    then the four waves in order;  a wave (or the whole first pass) may hold no inlier at all
    nq > n                          the tails of mask / q / t;  nq > 256: more than one stride of the block writing them
    iters larger than before        the RANSAC workspace of the scratch in use (the main one, or a pose alternate's) grows

CPU figures of the restatement (tests/test_planted_pnp_ref.py prints them; they are inputs' properties, not GPU results):
    ties                            60 correspondences, 10 noise-free inliers, 1025 hypotheses: first maximum at hypothesis 27 (tied with
                                    209), 272 (1001), 600 (753), 443 (586), 454 (998) -- thread 27 of pass 0 and one per wave of later passes
    refit, 0.3 px noise             moves the winner by 2.3e-3 .. 1.3e-2; summing in thread-strided order moves the restatement by at most
                                    3.9e-16, longdouble sums by at most 7.5e-16 (asserted below 1e-11)
    distance to the planted (R, t)  winner -> refit, largest |difference|: 6 inliers 1.2e-2 -> 4.8e-3; 257: 5.1e-3 -> 6.6e-4; 1024: 6.7e-3 ->
                                    2.0e-4; 2400: 2.2e-3 -> 2.6e-4; noise-free 6 / 7 of 12: 1.6e-7 -> 5.3e-8, 3.5e-7 -> 2.4e-7
    flags at (nq, M) = (600, 520)   cross-check 520 -> 480 matches, loop <= 48: 461, window (80, 60): 397, all three + ROI (3, 5): 358

Not covered here.  The dense arm of k_pnp_prep (bilinear lookup, status 1 / 2, flag bit 0): the slots planted here are sparse slots;
tests/test_gpu_planted_dense.py plants dense ones (a disparity image under the keypoints) and drives that arm.  Refit status -1: a winner with six inliers or more contains its own three non-collinear sample points, so
J^T J has full rank, and float32-finite inliers give finite float64 sums -- no honest input reaches it; it stays covered by
tests/test_pnp_refine_ref.py on the CPU and tests/test_pnp_pair_host.py on the odometer's side, and no hook forces it.

One child process per group of cases, VO355_LIB pointing at the test-only library; the cases are the parametrisation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted_pnp as PP                   # noqa: E402
from planted_pnp import PnpCase            # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_RT, BAR_REFIT = 1e-10, 1e-9            # the bars tests/test_gpu_pnp_pair.py holds the same two poses to
SCALARS = ("matches", "n", "flags", "best_iter", "best_count", "refine_status", "refine_steps")


# ------------------------------------------------------------------------------------------------ in the child process
def _small_context():
    from openvo_amd import _native
    ctx = _native.Context(0, 64, 64, 16, 4096)        # image size is irrelevant; kp_cap = 9216 >= 4096
    Q = np.eye(4)
    Q[3, 3] = 0.0; Q[2, 3] = 50.0; Q[3, 2] = 10.0
    ctx.set_Q(Q)
    return ctx


def _plant(ctx, c, sa=0, sb=1):
    c.build()
    ctx.plant_keypoints(sa, c.xy_a, c.dq, c.xyz_a, c.rd_a)
    ctx.plant_keypoints(sb, c.xy_b, c.dt, c.xyz_b, c.rd_b)


def _args(c, sa, sb):
    kw = dict(iters=c.iters, thr=PP.THR, seed=c.seed, refine=c.refine, want_matches=True, cross_check=c.cross)
    return (sa, sb, PP.RATIO, c.K4), kw


def _full(ctx, r, nq):
    """the record with mask / q / t as the step wrote them for ALL nq query keypoints (the binding cuts them at n)"""
    r = dict(r)
    for k, a in zip(("mask", "q", "t"), ctx._pnp_arrays):
        r[k] = a[:nq].copy()
    return r


def _poison(ctx):
    """nothing an earlier call left in the binding's output arrays can pass for this one's output"""
    for a in ctx._pnp_out(True)[1]:
        a[:] = 0x5A


def _sync(ctx, c, sa=0, sb=1):
    a, kw = _args(c, sa, sb)
    _poison(ctx)
    r = ctx.pnp_pair_window(*a, c.window, loop=c.loop, **kw) if c.flagged else ctx.pnp_pair(*a, **kw)
    return _full(ctx, r, c.nq)


def _begin(ctx, c, sa=0, sb=1):
    a, kw = _args(c, sa, sb)
    return ctx.pnp_pair_begin_window(*a, c.window, loop=c.loop, **kw) if c.flagged else ctx.pnp_pair_begin(*a, **kw)


def _end(ctx, c, ticket):
    _poison(ctx)
    return _full(ctx, ctx.pnp_pair_end(ticket, want_matches=True), c.nq)


def _same_record(a, b, what):
    for k in SCALARS:
        assert a[k] == b[k], "%s: %s %s != %s" % (what, k, a[k], b[k])
    for k in ("Rt", "Rt_refined", "mask", "q", "t"):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _hold_to_model(ctx, c, m, r):
    """one record (arrays of length nq) against the model -> the largest |Rt_refined - restatement|"""
    nq, n = c.nq, m["n"]
    assert (r["matches"], r["n"], r["flags"]) == (m["M"], n, 0), "(M, n, flags) = (%d, %d, %d), want (%d, %d, 0)" % (r["matches"], r["n"], r["flags"], m["M"], n)
    assert np.array_equal(r["q"][:n], m["q"]) and np.array_equal(r["t"][:n], m["t"]), "q / t differ from the model's compaction"
    assert (r["q"][n:] == -1).all() and (r["t"][n:] == -1).all(), "the tails of q / t are not -1"
    assert np.array_equal(r["mask"][:n], m["mask"]), "mask differs from the oracle's in %d places" % int((r["mask"][:n] != m["mask"]).sum())
    assert not r["mask"][n:].any(), "the tail of mask is not 0"
    assert (r["best_iter"], r["best_count"]) == (m["best_iter"], m["best_count"]), "best (%d, %d), want (%d, %d)" % (r["best_iter"], r["best_count"], m["best_iter"], m["best_count"])
    d = float(np.abs(r["Rt"] - m["Rt"]).max())
    assert d <= BAR_RT, "Rt differs from the oracle by %.3g" % d
    if n >= 4:
        ref = ctx.ransac_pnp(m["X"], m["uv"], c.K4, c.iters, PP.THR, c.seed)
        assert (ref["best_iter"], ref["best_count"]) == (r["best_iter"], r["best_count"]) and np.array_equal(ref["mask"], r["mask"][:n])
        assert np.array_equal(ref["Rt"], r["Rt"]), "Rt is not bit-identical with ransac_pnp on the compacted arrays"
    else:
        assert not r["Rt"].any()
    assert (r["refine_status"], r["refine_steps"]) == (m["status"], m["steps"]), "refit (status, steps) = (%d, %d), want (%d, %d)" % (
        r["refine_status"], r["refine_steps"], m["status"], m["steps"])
    if m["status"] == 1:
        assert np.array_equal(r["Rt_refined"], r["Rt"]), "status 1: Rt_refined must be Rt"
        return 0.0
    d64, dld = float(np.abs(r["Rt_refined"] - m["Rt64"]).max()), float(np.abs(r["Rt_refined"] - m["Rt_ld"]).max())
    assert d64 <= BAR_REFIT and dld <= BAR_REFIT, "Rt_refined differs from the restatement by %.3g (float64 sums) / %.3g (longdouble sums)" % (d64, dld)
    return max(d64, dld)


def _check_case(ctx, O, c):
    """plant, run the step both ways, hold it to the model -> the figures of the case"""
    m = c.model(O)
    _plant(ctx, c)
    if c.roi is not None:
        ctx.set_roi(*c.roi)
    try:
        r = _sync(ctx, c)
        r2 = _end(ctx, c, _begin(ctx, c))
    finally:
        if c.roi is not None:
            ctx.set_roi(0, 0, 64, 64)                  # (origin 0: the add in uv is a no-op again)
    fig = dict(nq=c.nq, M=r["matches"], n=r["n"], best_iter=r["best_iter"], best_count=r["best_count"], status=r["refine_status"], steps=r["refine_steps"])
    print("%s: (nq, M, n) = (%d, %d, %d) best %d @ %d refit %d / %d; want (M, n) = (%d, %d) best %d @ %d refit %d / %d" % (
        c.name, c.nq, r["matches"], r["n"], r["best_count"], r["best_iter"], r["refine_status"], r["refine_steps"],
        m["M"], m["n"], m["best_count"], m["best_iter"], m["status"], m["steps"]), flush=True)
    fig["dR"] = _hold_to_model(ctx, c, m, r)
    print("    largest |Rt_refined - restatement| = %.3g" % fig["dR"], flush=True)
    _same_record(r, r2, "pnp_pair and pnp_pair_begin / _end")
    return fig


def _run_cases(ctx, O, cases):
    out = {}
    for c in cases:
        try:
            out[c.name] = dict(ok=True, **_check_case(ctx, O, c))
        except AssertionError as e:                    # (anything else -- a native error status, a fault -- ends the child)
            out[c.name] = dict(ok=False, err=str(e)[:1500])
            print("%s: FAILED %s" % (c.name, out[c.name]["err"]), flush=True)
    return out


def _group_body(group):
    from oracle import oracle as O
    ctx = _small_context()
    out = _run_cases(ctx, O, PP.GROUPS[group])
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


TICKET_ITERS = ((64, 1025, 64, 4096, 1), (4096, 1, 1025, 64, 64))


def _ticket_pairs():
    return [PnpCase("pair0_nq303_M300", 303, 300, n_in=200, noise=0.3, refine=3), PnpCase("pair1_nq80_M70", 80, 70, n_in=40, noise=1.0, refine=0, bad=range(0, 70, 7)),
            PnpCase("pair2_nq1030_M1025", 1030, 1025, n_in=700, noise=0.3, refine=5)]


def _tickets_body():
    """five tickets with (64, 1025, 64, 4096, 1) hypotheses on three planted pairs of a FRESH context, ended in reverse order: every
    pose alternate meets its first step, two of them a larger one than the context's default workspace holds; a second round asks
    each alternate for another size.  Then the main scratch grows (nq = 4096, 20000 hypotheses) and a small step after it is exact."""
    import copy
    from oracle import oracle as O
    ctx = _small_context()
    pairs = _ticket_pairs()
    for k, c in enumerate(pairs):
        _plant(ctx, c, 2 * k, 2 * k + 1)
    out = {}
    for rnd, iters in enumerate(TICKET_ITERS):
        steps = []
        for k, it in enumerate(iters):
            c = copy.copy(pairs[k % 3])
            c.iters, c._model, c.name = it, None, "round%d_ticket%d_%s_iters%d" % (rnd, k, pairs[k % 3].name, it)
            steps.append((c, 2 * (k % 3), 2 * (k % 3) + 1))
        tickets = [_begin(ctx, c, sa, sb) for c, sa, sb in steps]
        assert len(set(tickets)) == len(tickets)
        got = {}
        for (c, sa, sb), tk in reversed(list(zip(steps, tickets))):
            got[c.name] = _end(ctx, c, tk)
        for c, sa, sb in steps:
            try:
                r = got[c.name]
                dR = _hold_to_model(ctx, c, c.model(O), r)
                _same_record(r, _sync(ctx, c, sa, sb), "the ticket and the synchronous step")
                out[c.name] = dict(ok=True, n=r["n"], best_iter=r["best_iter"], best_count=r["best_count"], dR=dR)
                print("%s: n %d best %d @ %d, largest |Rt_refined - restatement| = %.3g" % (c.name, r["n"], r["best_count"], r["best_iter"], dR), flush=True)
            except AssertionError as e:
                out[c.name] = dict(ok=False, err=str(e)[:1500])
                print("%s: FAILED %s" % (c.name, out[c.name]["err"]), flush=True)
    out.update(_run_cases(ctx, O, [PnpCase("grow_main_nq4096_M1025_iters20000", 4096, 1025, n_in=700, noise=1.0, iters=20000, refine=3),
                                   PnpCase("small_step_after_the_growth", 67, 64, n_in=45, noise=1.0, refine=2)]))
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


TICKET_NAMES = ["round%d_ticket%d_%s_iters%d" % (rnd, k, _ticket_pairs()[k % 3].name, it) for rnd, iters in enumerate(TICKET_ITERS) for k, it in enumerate(iters)] + \
               ["grow_main_nq4096_M1025_iters20000", "small_step_after_the_growth"]


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    """run tests.test_gpu_planted_pnp.<body> once in a process of its own against the test-only library -> its result dict"""
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_planted_pnp as t; t.%s" % body], cwd=ROOT,
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


@pytest.mark.parametrize("group,name", PP.ALL_CASES, ids=["%s-%s" % gc for gc in PP.ALL_CASES])
def test_planted_pnp_regime(group, name):
    res = _child("_group_body(%r)" % group)[name]
    assert res["ok"], res["err"]
    print("%s: (nq, M, n, best_iter, best_count, refit status / steps) = (%d, %d, %d, %d, %d, %d / %d), largest |Rt_refined - restatement| = %.3g" % (
        name, res["nq"], res["M"], res["n"], res["best_iter"], res["best_count"], res["status"], res["steps"], res["dR"]))


@pytest.mark.parametrize("name", TICKET_NAMES)
def test_tickets_and_workspace_growth(name):
    res = _child("_tickets_body()")[name]
    assert res["ok"], res["err"]
    print("%s: n %d best %d @ %d, largest |Rt_refined - restatement| = %.3g" % (name, res["n"], res["best_count"], res["best_iter"], res["dR"]))
