"""The dense direct alignment on the device (k_direct_align behind vo_direct_align, csrc/direct.hip) held to its restatement
(tests/direct_ref.py) on the planted cases of tests/direct_cases.py, and StereoOdometer(direct_refine=True) on the corridor.

    matrix         every case of direct_cases.CASES, planted into two dense slots of the test-only library (plant_dense_pair):
                   status, iterations completed, s and every per-level count EXACTLY (tests/test_direct_ref.py asserts the decision
                   margin that makes them comparable); the pose within 1e-9 (largest absolute entry difference: the project's bar for a
                   pose through reordered float64 sums); sum w r^2 of every level's first and last iteration and of the last
                   linearisation and the 21 sums of H within 1e-9 relative, each to its own magnitude; the six sums of g within
                   1e-9 of the sum of their terms' magnitudes (direct_ref's sums_abs), and g ALONE: g = sum w j r cancels to zero as the
                   iteration converges -- that is what converging means, to about 1e-13 of its terms here -- so relative to |g| no
                   two orders of summation agree: on the CPU, numpy's pairwise float64 sum and its np.longdouble sum of the same
                   terms differ by more than |g| itself on case levels4.  Every figure is printed before it is asserted, g's plain
                   relative difference too; where a plain relative difference exceeds 1e-9 the np.longdouble run of the same sums
                   is added and the report says which of the two float64 sides is nearer to it.
    repeatability  the same call twice: a bit-identical record
    misuse         one test per error of include/vo355.h: VO_E_ARG (ranges, non-finite Rt0 / K4), VO_E_STATE (no disparity, no
                   image, a sparse slot, two sizes), VO_E_SWEEP (the forced give-up of the test-only library: VO_FAULT_SWEEP)
    the odometer   corridor T0 (320 x 240, D 32), six frames, both pose methods: run() equals update() bit for bit, direct_status 0 on
                   every accepted frame, the refined chain ends nearer to the ground truth than the unrefined chain of the same
                   process (the Umeyama case under a guard as wide as its feature poses' error: see the comment at the test), an
                   odometer without the keyword is bit-identical to the unrefined chain, a guard of (0, 0) leaves every pose the
                   feature pose; and the Umeyama odometer under the DEFAULT guard: run() equals update(), direct_status 0 on every
                   accepted frame, poses both taken and refused (no claim about its end point: the constructor's text says why).

The planted cases run in ONE child process on the test-only library (VO355_LIB); the cases are the parametrisation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_cases as DC                  # noqa: E402
import direct_ref as DR                    # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_ARG, VO_E_STATE, VO_E_SWEEP = -1, -3, -6
BAR = 1e-9


# ------------------------------------------------------------------------------------------------ in the child process
def _run(out, name, fn):
    try:
        out[name] = dict(ok=True, **(fn() or {}))
    except AssertionError as e:                        # (anything else -- a native error status, a fault -- ends the child)
        out[name] = dict(ok=False, err=str(e)[:3000])
        print("%s: FAILED %s" % (name, out[name]["err"]), flush=True)


def _context(roi=None):
    from openvo_amd import _native
    ctx = _native.Context(0, 128, 96, 16, 256)
    if roi is not None:
        ctx.set_roi(*roi)                              # (before anything is planted, and never changed afterwards)
    return ctx


def _plant(ctx, slot, img, disp):
    ctx.plant_dense_pair(slot, img, disp, np.float32([[1, 1]]))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(den > 0, np.abs(a - b) / np.where(den > 0, den, 1.0), 0.0))) if a.size else 0.0


def _same_record(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _compare(case, got, want):
    """every figure printed, then asserted"""
    A, B, disp, Q, K4, Rt0, _ = case.build()
    ints = ("status", "iters_done", "s", "selected", "n_first", "n_last", "count")
    d_pose = float(np.abs(got["Rt"] - want["Rt"]).max())
    r_wr2 = max(_rel(got["wr2_first"], want["wr2_first"]), _rel(got["wr2_last"], want["wr2_last"]), _rel(got["wr2"], want["wr2"]))
    scale = np.where(want["sums_abs"] > 0, want["sums_abs"], 1.0)
    r_g = float(np.max((np.abs(got["sums"] - want["sums"]) / scale)[21:]))
    plain = np.abs(got["sums"] - want["sums"]) / np.where(np.abs(want["sums"]) > 0, np.abs(want["sums"]), 1.0)
    r_H = float(plain[:21].max())
    print("%s: status %d / %d, iterations %d / %d, s %s, selected %s, first %s, last %s | pose %.2e, wr2 %.2e, H %.2e relative, g %.2e of "
          "its terms' magnitudes (g plain relative: %.2e)"
          % (case.name, got["status"], want["status"], got["iters_done"], want["iters_done"], got["s"].tolist(), got["selected"].tolist(),
             got["n_first"].tolist(), got["n_last"].tolist(), d_pose, r_wr2, r_H, r_g, float(plain[21:].max())), flush=True)
    if plain.max() > BAR:                              # the referee: the same sums in extended precision
        ld = DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, sum_dtype=np.longdouble, **case.kw)
        k = int(np.argmax(plain))
        e_dev, e_ref = abs(got["sums"][k] - ld["sums"][k]), abs(want["sums"][k] - ld["sums"][k])
        print("    sum %d (%s): device %.17g, float64 restatement %.17g, np.longdouble %.17g, magnitudes %.3g: the %s is nearer (%.2e against %.2e)"
              % (k, "H" if k < 21 else "g", got["sums"][k], want["sums"][k], ld["sums"][k], want["sums_abs"][k],
                 "device" if e_dev <= e_ref else "restatement", e_dev, e_ref), flush=True)
    for k in ints:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), "%s: %s is %s, the restatement's %s" % (case.name, k, got[k], want[k])
    assert got["status"] == case.expect["status"]
    assert d_pose <= BAR, "%s: the pose differs by %.3e" % (case.name, d_pose)
    assert r_wr2 <= BAR, "%s: sum w r^2 differs by %.3e relative" % (case.name, r_wr2)
    assert r_H <= BAR, "%s: a sum of H differs by %.3e relative" % (case.name, r_H)
    assert r_g <= BAR, "%s: a sum of g differs by %.3e of its terms' magnitudes" % (case.name, r_g)
    return dict(pose=d_pose, wr2=r_wr2, H=r_H, g=r_g)


def _matrix_body():
    out, plain_ctx = {}, _context()
    for case in DC.CASES:
        def check(case=case):
            A, B, disp, Q, K4, Rt0, _ = case.build()
            ctx = plain_ctx if case.roi is None else _context(case.roi)
            ctx.set_Q(Q)
            _plant(ctx, 0, A, disp)
            _plant(ctx, 1, B, disp)
            got = ctx.direct_align(0, 1, K4, Rt0, **case.kw)
            again = ctx.direct_align(0, 1, K4, Rt0, **case.kw)
            if ctx is not plain_ctx:
                ctx.close()
            want = DR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **case.kw)
            assert want["margin"] >= DC.MARGIN
            res = _compare(case, got, want)
            assert _same_record(got, again), "%s: the same call twice gave two records" % case.name
            if case.expect.get("huber"):               # (the weights act on the device too: without them the sums are others)
                assert want["n_huber"] > 0
            return res
        _run(out, case.name, check)
    plain_ctx.close()
    print("DIRECT-RESULT " + json.dumps(out))


def _misuse_body():
    from openvo_amd import _native
    case = DC.BY_NAME["small"]
    A, B, disp, Q, K4, Rt0, _ = case.build()
    out, ctx = {}, _context()
    ctx.set_Q(Q)
    _plant(ctx, 0, A, disp)
    _plant(ctx, 1, B, disp)
    good = ctx.direct_align(0, 1, K4, Rt0, **case.kw)
    assert good["status"] == 0

    def refused(code, slot_a=0, slot_b=1, K=K4, Rt=Rt0, raw=None, **kw):
        try:
            if raw is not None:                        # past the Python layer's own checks: the library's
                rec = _native.DirectRec()
                prm = dict(case.kw, **raw)
                rc = ctx._lib.vo_direct_align(ctx._h, slot_a, slot_b, _native._p(np.float64(K)), _native._p(np.float64(Rt).reshape(12)),
                                              prm["levels"], prm["iters"], prm["max_points"], prm["grad_min"], prm["huber"], prm["dmin"], prm["dmax"],
                                              prm["z_min"], prm["min_pixels"], __import__("ctypes").byref(rec))
                assert rc == code, "status %d, expected %d (%r)" % (rc, code, raw)
                assert rec.levels == 0 and not any(rec.Rt[:]), "a refused call wrote its record"
                return
            ctx.direct_align(slot_a, slot_b, K, Rt, **dict(case.kw, **kw))
        except _native.VoError as e:
            assert e.code == code, "%s, expected %d" % (e, code)
            return
        raise AssertionError("not refused: %r" % (kw,))

    def arg():
        for raw in (dict(levels=0), dict(levels=5), dict(iters=0), dict(iters=21), dict(max_points=0), dict(grad_min=-1), dict(grad_min=256),
                    dict(huber=0.0), dict(huber=float("nan")), dict(dmin=0.0), dict(dmin=13.0, dmax=12.0), dict(dmax=float("inf")),
                    dict(z_min=-1.0), dict(min_pixels=5)):
            refused(VO_E_ARG, raw=raw)
        bad = np.array(Rt0, np.float64)
        bad[1, 2] = np.nan
        refused(VO_E_ARG, Rt=bad, raw={})
        refused(VO_E_ARG, K=(K4[0], K4[1], np.inf, K4[3]), raw={})
        refused(VO_E_ARG, K=(0.0, K4[1], K4[2], K4[3]), raw={})
        refused(VO_E_ARG, slot_a=-1, raw={})
        refused(VO_E_ARG, slot_b=_native.VO_NUM_SLOTS, raw={})

    def state():
        ctx.upload_pair(2, A, A, True)                 # an image pair, no disparity
        refused(VO_E_STATE, slot_a=2)
        refused(VO_E_STATE, slot_b=3)                  # an empty slot: no image
        refused(VO_E_STATE, slot_a=3)
        ctx.upload_pair(4, A, A, True)                 # a sparse slot: its keypoints carry depth
        ctx.plant_keypoints(4, np.float32([[5, 5]]), np.zeros((1, 32), np.uint8), np.float32([[0, 0, 2]]))
        refused(VO_E_STATE, slot_a=4)
        big = DC.BY_NAME["levels3"].build()
        _plant(ctx, 5, big[1], big[2])                 # another size
        refused(VO_E_STATE, slot_b=5)
        again = ctx.direct_align(0, 1, K4, Rt0, **case.kw)      # the refusals touched nothing
        assert _same_record(good, again)

    def no_q():
        c2 = _context()
        _plant(c2, 0, A, disp)
        _plant(c2, 1, B, disp)
        try:
            c2.direct_align(0, 1, K4, Rt0, **case.kw)
        except _native.VoError as e:
            assert e.code == VO_E_STATE
        else:
            raise AssertionError("no vo_set_Q: not refused")
        c2.close()

    def sweep():
        from openvo_amd.synth import Corridor
        c = Corridor("T0")
        os.environ["VO_FAULT_SWEEP"] = "1"             # the first diagonal sweep of the next context gives up its hand-offs
        c3 = _native.Context(0, c.w, c.h, c.D, 256)
        del os.environ["VO_FAULT_SWEEP"]
        c3.set_sgbm(c.sgbm_params())
        c3.set_Q(c.Q())
        for slot, k in ((0, 0), (1, 1)):
            c3.upload_pair(slot, *c.pair(k), True)
            c3.sgbm_compute(slot)
        try:
            c3.direct_align(0, 1, (c.f, c.f, c.cx, c.cy))
        except _native.SweepTimeout as e:
            assert e.code == VO_E_SWEEP
        else:
            raise AssertionError("slot a's disparity is undefined: not refused")
        r = c3.direct_align(1, 0, (c.f, c.f, c.cx, c.cy))       # slot 1's disparity is sound (b's is not read): not refused
        assert r["status"] in (0, 2, -1)
        c3.close()

    for name, fn in (("arg", arg), ("state", state), ("no_q", no_q), ("sweep", sweep)):
        _run(out, name, fn)
    ctx.close()
    print("DIRECT-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ the tests
_RESULTS, _STOPPED = {}, []


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_direct as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIRECT-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("DIRECT-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("DIRECT-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_matches_the_restatement_and_repeats(name):
    res = _child("_matrix_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", ("arg", "state", "no_q", "sweep"))
def test_misuse(name):
    res = _child("_misuse_body()")[name]
    assert res["ok"], res["err"]


# ---- the odometer ------------------------------------------------------------------------------------------------------------------------
FRAMES = 6


@pytest.fixture(scope="module")
def rig():
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    c = Corridor("T0")
    cx = _native.Context(0, c.w, c.h, c.D, 500)
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=cx)
    yield dict(ctx=cx, cam=cam, pairs=c.pairs(0, FRAMES), gt=c.gt_pose(FRAMES - 1))
    cx.close()


def _odo(cam, method, **kw):
    """the odometer of smoke(): the clique and outlier filters on (pose_method="umeyama" without them is decimetres off per pair
    on this corridor, so that the guard -- rightly -- takes none of the refined poses and the two chains are one)"""
    from openvo_amd import StereoOdometer
    return StereoOdometer(cam, preprocessed_frames=True, pose_method=method, rigidity_threshold=0.1, outlier_threshold=0.02, **kw)


def _updates(o, pairs):
    out = []
    for L, R in pairs:
        ok = o.update(L, R)
        out.append((ok, o.skip_cause, o.c_T_w.copy(), getattr(o, "direct_status", None), getattr(o, "direct_accepted", None)))
    o.reset_lookahead()
    return out


def _end_error(o, gt):
    return float(np.linalg.norm(np.linalg.inv(o.c_T_w)[:3, 3] - gt[:3, 3]))


# The guard bounds what the alignment may move a feature pose by, so it has to be at least as wide as the feature pose's own error,
# or it refuses exactly the corrections that matter.  Against the ground truth of this corridor (320 x 240, D = 32) the filtered
# 3-D / 3-D Umeyama poses of the five pairs are 0.053 / 0.293 / 0.058 / 0.192 / 0.308 m (0.010 / 0.042 / 0.008 / 0.029 / 0.051 rad)
# off -- a property of the feature path and the scene, measured before anything is refined -- while the alignment started from
# them ends 1.0 - 2.8 mm off in every pair.  The default guard (0.1 m, 0.05 rad) therefore refuses three of the five corrections,
# and the two it takes break the cancellation among the unrefined pairs' errors (end point 0.3197 m unrefined, 0.3655 m with two
# poses taken).  The Umeyama case runs with (0.5 m, 0.1 rad): wider than that feature error with room to spare, half the distance
# gate (1 m) and a tenth of the rotation gate (pi / 3).  The PnP poses are 0.6 - 7.4 cm off: the default guard.
@pytest.mark.parametrize("method,guard", (("umeyama", (0.5, 0.1)), ("pnp", (0.1, 0.05))))
def test_odometer_refines_and_run_equals_update(rig, method, guard):
    cam, pairs = rig["cam"], rig["pairs"]
    plain = _odo(cam, method)
    base = _updates(plain, pairs)
    a = _odo(cam, method, direct_refine=True, direct_guard=guard)
    want = _updates(a, pairs)
    b = _odo(cam, method, direct_refine=True, direct_guard=guard)
    got = [(ok, b.skip_cause, b.c_T_w.copy(), b.direct_status, b.direct_accepted) for ok in b.run(iter(pairs))]
    b.reset_lookahead()
    assert len(got) == len(want) == FRAMES
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and g[3] == w[3] and g[4] == w[4], k
    taken = accepted = 0
    for k, w in enumerate(want[1:], 1):
        if w[0]:
            assert w[3] == 0, (k, w[3])                # every accepted frame: all iterations ran
            accepted += 1
            taken += bool(w[4])
    assert accepted >= 3 and taken >= 1 and a.pose_information is not None and a.pose_information.shape == (6, 6)
    assert np.array_equal(a.pose_information, a.pose_information.T) and (np.linalg.eigvalsh(a.pose_information) > 0).all()
    e_plain, e_ref = _end_error(plain, rig["gt"]), _end_error(a, rig["gt"])
    print("%s: end-point error after %d frames %.4f m unrefined, %.4f m refined (%d of %d poses taken from the alignment)"
          % (method, FRAMES, e_plain, e_ref, taken, FRAMES - 1))
    assert e_ref < e_plain
    # an odometer without the keyword is what it was: bit-identical to the unrefined chain, before and after the refined ones ran
    again = _updates(_odo(cam, method), pairs)
    for g, w in zip(again, base):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2])
    # a guard of (0, 0) leaves every pose the feature pose
    z = _odo(cam, method, direct_refine=True, direct_guard=(0, 0))
    zero = _updates(z, pairs)
    for g, w in zip(zero, base):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and not g[4]
    assert z.direct_status == 0 and z.pose_information is None


def test_umeyama_under_the_default_guard_runs_and_refuses(rig):
    """The shipped default guard with pose_method="umeyama": sized for PnP-grade starts, it refuses the corrections of the pairs whose
    feature pose is more than 0.1 m off (the constructor's text warns), so nothing is claimed about the end point -- only that the
    mode runs: run() equals update() bit for bit, every accepted frame's step ran all its iterations, some refined poses are taken
    and some refused, and pose_information is the delivered pose's or None."""
    cam, pairs = rig["cam"], rig["pairs"]
    a = _odo(cam, "umeyama", direct_refine=True)
    want, infos = [], []
    for L, R in pairs:
        ok = a.update(L, R)
        want.append((ok, a.skip_cause, a.c_T_w.copy(), a.direct_status, a.direct_accepted))
        infos.append(a.pose_information)
    a.reset_lookahead()
    b = _odo(cam, "umeyama", direct_refine=True)
    got = [(ok, b.skip_cause, b.c_T_w.copy(), b.direct_status, b.direct_accepted) for ok in b.run(iter(pairs))]
    b.reset_lookahead()
    assert len(got) == len(want) == FRAMES
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and g[3] == w[3] and g[4] == w[4], k
    accepted = [w for w in want[1:] if w[0]]
    assert len(accepted) >= 3 and all(w[3] == 0 for w in accepted)
    taken = [bool(w[4]) for w in want[1:]]
    print("umeyama, default guard: refined poses taken per pair %s" % taken)
    assert any(taken) and not all(taken)
    for w, info in zip(want[1:], infos[1:]):
        if w[0]:
            assert (info is not None) == bool(w[4])
