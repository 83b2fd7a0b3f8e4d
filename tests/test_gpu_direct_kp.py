"""The patch alignment on the device (k_direct_align_kp behind vo_direct_align_kp, csrc/direct.hip) held to its restatement
(tests/direct_kp_ref.py) on the planted cases of tests/direct_kp_cases.py, and StereoOdometer(patch_refine=True) on the corridor.

    matrix         every case of direct_kp_cases.CASES: slot a is upload_pair(A, A) + plant_keypoints of the test-only library, slot b
                   upload_pair(B, B).  Status, iterations completed, the keypoints in use and every per-level count EXACTLY
                   (tests/test_direct_kp_ref.py asserts the decision margin that makes them comparable); the pose within 1e-9; sum
                   w r^2 of every level's first and last iteration and of the last linearisation and the 21 sums of H within 1e-9
                   relative, each to its own magnitude; the six sums of g within 1e-9 of the sum of their terms' magnitudes (g cancels
                   to zero as the iteration converges: tests/test_gpu_direct.py says why it has no relative bar of its own).  These are
                   the bars of tests/test_gpu_direct.py.  Every figure is printed before it is asserted, and the maxima over the cases.
    repeatability  the same call twice: a bit-identical record
    misuse         one test per error: VO_E_ARG (ranges, patch=4, non-finite Rt0 / K4), VO_E_STATE (a dense slot a, an empty slot b,
                   two sizes), no vo_set_Q; a refused call writes no record
    the odometer   corridor C1 (640 x 480), frames 0 - 7, 500 features, depth="sparse", pose_method="pnp" -- the corridor and settings
                   of tests/test_gpu_sparse_stereo.py: run() equals update() bit for bit; patch_guard=(0, 0) and the keyword off are
                   bit-identical to the unrefined chain; the refined chain ends nearer to the ground truth than the unrefined one.

Measured on one MI355X over the 24 cases: every integer field equal; the pose at most 8.5e-16 (3.9e-12 on the diverging
`starved_midway`), sum w r^2 8.1e-14 relative (4.1e-11), H 7.7e-14 relative (5.5e-11), g 1.8e-13 of its terms' magnitudes (5.0e-12).  The
odometer on C1: 0.0441 m unrefined, 0.0026 m refined, 7 of 7 refined poses taken -- the CPU chain's figures for RANSAC seed 4321.

The planted cases run in ONE child process on the test-only library (VO355_LIB); the cases are the parametrisation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_kp_cases as KC               # noqa: E402
import direct_kp_ref as KR                 # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_ARG, VO_E_STATE = -1, -3
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
    ctx = _native.Context(0, 128, 96, 16, 512)
    if roi is not None:
        ctx.set_roi(*roi)                              # (before anything is planted, and never changed afterwards)
    return ctx


def _plant(ctx, A, B, xy, xyz, slot_a=0, slot_b=1):
    ctx.upload_pair(slot_a, A, A, True)
    ctx.plant_keypoints(slot_a, xy, np.zeros((len(xy), 32), np.uint8), xyz)
    ctx.upload_pair(slot_b, B, B, True)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(den > 0, np.abs(a - b) / np.where(den > 0, den, 1.0), 0.0))) if a.size else 0.0


def _same_record(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def _compare(case, got, want):
    """every figure printed, then asserted"""
    A, B, xy, xyz, Q, K4, Rt0, _ = case.build()
    ints = ("status", "iters_done", "keypoints", "selected", "n_first", "n_last", "count", "patch")
    d_pose = float(np.abs(got["Rt"] - want["Rt"]).max())
    r_wr2 = max(_rel(got["wr2_first"], want["wr2_first"]), _rel(got["wr2_last"], want["wr2_last"]), _rel(got["wr2"], want["wr2"]))
    scale = np.where(want["sums_abs"] > 0, want["sums_abs"], 1.0)
    r_g = float(np.max((np.abs(got["sums"] - want["sums"]) / scale)[21:]))
    plain = np.abs(got["sums"] - want["sums"]) / np.where(np.abs(want["sums"]) > 0, np.abs(want["sums"]), 1.0)
    r_H = float(plain[:21].max())
    print("%s: status %d / %d, iterations %d / %d, keypoints %s, selected %s, first %s, last %s | pose %.2e, wr2 %.2e, H %.2e relative, g %.2e "
          "of its terms' magnitudes (g plain relative: %.2e)"
          % (case.name, got["status"], want["status"], got["iters_done"], want["iters_done"], got["keypoints"].tolist(), got["selected"].tolist(),
             got["n_first"].tolist(), got["n_last"].tolist(), d_pose, r_wr2, r_H, r_g, float(plain[21:].max())), flush=True)
    if plain.max() > BAR:                              # the referee: the same sums in extended precision
        ld = KR.align(A, B, xy, xyz, Q, K4, Rt0, roi=case.roi, sum_dtype=np.longdouble, **case.kw)
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
    for case in KC.CASES:
        def check(case=case):
            A, B, xy, xyz, Q, K4, Rt0, _ = case.build()
            ctx = plain_ctx if case.roi is None else _context(case.roi)
            ctx.set_Q(Q)
            _plant(ctx, A, B, xy, xyz)
            got = ctx.direct_align_kp(0, 1, K4, Rt0, **case.kw)
            again = ctx.direct_align_kp(0, 1, K4, Rt0, **case.kw)
            if ctx is not plain_ctx:
                ctx.close()
            want = KR.align(A, B, xy, xyz, Q, K4, Rt0, roi=case.roi, **case.kw)
            assert want["margin"] >= KC.MARGIN
            res = _compare(case, got, want)
            assert _same_record(got, again), "%s: the same call twice gave two records" % case.name
            if case.expect.get("huber"):               # (the weights act on the device too: without them the sums are others)
                assert want["n_huber"] > 0
            return res
        _run(out, case.name, check)
    plain_ctx.close()
    done = [v for v in out.values() if v["ok"]]
    if done:
        print("maxima over %d cases: pose %.2e, wr2 %.2e, H %.2e, g %.2e" % ((len(done),) + tuple(max(v[k] for v in done) for k in ("pose", "wr2", "H", "g"))))
    print("DIRECT-KP-RESULT " + json.dumps(out))


def _misuse_body():
    import ctypes
    from openvo_amd import _native
    case = KC.BY_NAME["p3_levels2"]
    A, B, xy, xyz, Q, K4, Rt0, _ = case.build()
    out, ctx = {}, _context()
    ctx.set_Q(Q)
    _plant(ctx, A, B, xy, xyz)
    good = ctx.direct_align_kp(0, 1, K4, Rt0, **case.kw)
    assert good["status"] == 0

    def refused(code, slot_a=0, slot_b=1, K=K4, Rt=Rt0, c=None, **raw):
        """past the Python layer's own checks: the library's status, and a record it did not write"""
        c = c or ctx
        rec = _native.DirectRec()
        prm = dict(case.kw, **raw)
        rc = c._lib.vo_direct_align_kp(c._h, slot_a, slot_b, _native._p(np.float64(K)), _native._p(np.float64(Rt).reshape(12)), prm["levels"],
                                       prm["iters"], prm["patch"], prm["grad_min"], prm["huber"], prm["z_min"], prm["min_pixels"], ctypes.byref(rec))
        assert rc == code, "status %d, expected %d (%r)" % (rc, code, raw)
        assert rec.levels == 0 and rec.pad == 0 and not any(rec.Rt[:]), "a refused call wrote its record"

    def untouched():
        assert _same_record(good, ctx.direct_align_kp(0, 1, K4, Rt0, **case.kw)), "a refusal touched the slots"

    def arg():
        for raw in (dict(levels=0), dict(levels=5), dict(iters=0), dict(iters=21), dict(grad_min=-1), dict(grad_min=256), dict(huber=0.0),
                    dict(huber=float("nan")), dict(z_min=-1.0), dict(z_min=float("inf")), dict(min_pixels=5)):
            refused(VO_E_ARG, **raw)
        bad = np.array(Rt0, np.float64)
        bad[1, 2] = np.nan
        refused(VO_E_ARG, Rt=bad)
        refused(VO_E_ARG, K=(K4[0], K4[1], np.inf, K4[3]))
        refused(VO_E_ARG, K=(0.0, K4[1], K4[2], K4[3]))
        refused(VO_E_ARG, slot_a=-1)
        refused(VO_E_ARG, slot_b=_native.VO_NUM_SLOTS)
        untouched()

    def patch4():
        for p in (4, 0, 1, 2, 6, 9, -3):
            refused(VO_E_ARG, patch=p)
        untouched()

    def dense_a():
        disp = np.full(A.shape, 16 * 12, np.int16)
        ctx.plant_dense_pair(2, A, disp, np.float32([[5, 5]]))        # an image, a disparity, keypoints without depth
        refused(VO_E_STATE, slot_a=2)
        ctx.upload_pair(3, A, A, True)                                # an image pair and nothing else
        refused(VO_E_STATE, slot_a=3)
        r = ctx.direct_align_kp(0, 2, K4, Rt0, **case.kw)             # as slot b a dense slot is fine: only its image is read
        assert r["status"] in (0, 2, -1)
        untouched()

    def empty_b():
        refused(VO_E_STATE, slot_b=5)                                 # an empty slot: no image
        refused(VO_E_STATE, slot_a=5)
        untouched()

    def shape():
        big = KC.BY_NAME["p5_levels3"].build()
        ctx.upload_pair(6, big[1], big[1], True)                      # another size
        refused(VO_E_STATE, slot_b=6)
        untouched()

    def no_q():
        c2 = _context()
        _plant(c2, A, B, xy, xyz)
        refused(VO_E_STATE, c=c2)
        try:
            c2.direct_align_kp(0, 1, K4, Rt0, **case.kw)
        except _native.VoError as e:
            assert e.code == VO_E_STATE
        else:
            raise AssertionError("no vo_set_Q: not refused")
        Q0 = np.array(Q, np.float64)
        Q0[2, 3] = 0.0                                                # a Q whose [2][3] is zero: s_i has no value
        c2.set_Q(Q0)
        refused(VO_E_STATE, c=c2)
        c2.close()

    for name, fn in (("arg", arg), ("patch4", patch4), ("dense_a", dense_a), ("empty_b", empty_b), ("shape", shape), ("no_q", no_q)):
        _run(out, name, fn)
    ctx.close()
    print("DIRECT-KP-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ the tests
_RESULTS, _STOPPED = {}, []


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_direct_kp as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIRECT-KP-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("DIRECT-KP-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("DIRECT-KP-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", [c.name for c in KC.CASES])
def test_matches_the_restatement_and_repeats(name):
    res = _child("_matrix_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", ("arg", "patch4", "dense_a", "empty_b", "shape", "no_q"))
def test_misuse(name):
    res = _child("_misuse_body()")[name]
    assert res["ok"], res["err"]


# ---- the odometer ------------------------------------------------------------------------------------------------------------------------
FRAMES = 8


@pytest.fixture(scope="module")
def rig():
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    cx = _native.Context(0, c.w, c.h, c.D, 500)
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=cx)
    gt = np.linalg.inv(type(c).gt_pose(0)) @ type(c).gt_pose(FRAMES - 1)
    yield dict(ctx=cx, cam=cam, pairs=c.pairs(0, FRAMES), gt=gt)
    cx.close()


def _odo(cam, method, **kw):
    from openvo_amd import StereoOdometer
    return StereoOdometer(cam, preprocessed_frames=True, depth="sparse", pose_method=method, **kw)


@pytest.mark.parametrize("name,method,kw", (("umeyama", "umeyama", {}), ("klt", "pnp", dict(match="klt")),
                                            ("klt_fused", "pnp", dict(match="klt", klt_fused=True))))
def test_other_routes_to_the_gate_run_equals_update(rig, name, method, kw):
    """The other routes by which a pose reaches _gate in sparse mode -- the 3-D / 3-D fit (point_cloud_transform), the composed
    Lucas-Kanade step, and the fused one whose steps run() begins ahead: run() equals update() bit for bit, every pose that reached
    the gate was refined (a status is recorded, 0 on every accepted frame), and with the keyword off the chain is what it was."""
    cam, pairs = rig["cam"], rig["pairs"]
    base = _updates(_odo(cam, method, **kw), pairs)
    a = _odo(cam, method, patch_refine=True, **kw)
    want = _updates(a, pairs)
    b = _odo(cam, method, patch_refine=True, **kw)
    got = [(ok, b.skip_cause, b.c_T_w.copy(), b.patch_status, b.patch_accepted) for ok in b.run(iter(pairs))]
    b.reset_lookahead()
    assert len(got) == len(want) == FRAMES
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and g[3] == w[3] and g[4] == w[4], (name, k)
    accepted = [w for w in want[1:] if w[0]]
    taken = sum(bool(w[4]) for w in accepted)
    e_plain = float(np.linalg.norm(np.linalg.inv(base[-1][2])[:3, 3] - rig["gt"][:3, 3]))
    print("%s: %d of %d frames accepted, %d refined poses taken; end-point error %.4f m unrefined, %.4f m refined"
          % (name, len(accepted), FRAMES - 1, taken, e_plain, _end_error(a, rig["gt"])))
    assert len(accepted) >= 3 and all(w[3] == 0 for w in accepted)
    if name == "klt_fused":
        assert b.klt_ahead > 0                         # (steps were collected from tickets begun ahead, and refined behind them)
    again = _updates(_odo(cam, method, **kw), pairs)
    for g, w in zip(again, base):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2])


def _updates(o, pairs):
    out = []
    for L, R in pairs:
        ok = o.update(L, R)
        out.append((ok, o.skip_cause, o.c_T_w.copy(), getattr(o, "patch_status", None), getattr(o, "patch_accepted", None)))
    o.reset_lookahead()
    return out


def _end_error(o, gt):
    return float(np.linalg.norm(np.linalg.inv(o.c_T_w)[:3, 3] - gt[:3, 3]))


def test_odometer_refines_and_run_equals_update(rig):
    """pose_method="pnp" under the default guard (its poses are centimetres off: the guard's size)"""
    cam, pairs = rig["cam"], rig["pairs"]
    plain = _odo(cam, "pnp")
    base = _updates(plain, pairs)
    a = _odo(cam, "pnp", patch_refine=True)
    want = _updates(a, pairs)
    b = _odo(cam, "pnp", patch_refine=True)
    got = [(ok, b.skip_cause, b.c_T_w.copy(), b.patch_status, b.patch_accepted) for ok in b.run(iter(pairs))]
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
    r = a.patch_record
    print("last step: keypoints %s, selected %s, first %s, last %s" % (r["keypoints"].tolist(), r["selected"].tolist(), r["n_first"].tolist(), r["n_last"].tolist()))
    assert r["patch"] == 5 and r["iters_done"] == 12 and (r["keypoints"] > 0).all()
    assert accepted >= 6 and taken >= 4 and a.pose_information is not None        # (7 of 7 taken when measured: half, rounded up) and a.pose_information.shape == (6, 6)
    assert np.array_equal(a.pose_information, a.pose_information.T) and (np.linalg.eigvalsh(a.pose_information) > 0).all()
    e_plain, e_ref = _end_error(plain, rig["gt"]), _end_error(a, rig["gt"])
    print("pnp: end-point error after %d frames %.4f m unrefined, %.4f m refined (%d of %d poses taken from the alignment)"
          % (FRAMES, e_plain, e_ref, taken, FRAMES - 1))
    assert e_ref < e_plain
    # an odometer without the keyword is what it was: bit-identical to the unrefined chain, before and after the refined ones ran
    again = _updates(_odo(cam, "pnp"), pairs)
    for g, w in zip(again, base):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2])
    # a guard of (0, 0) leaves every pose the feature pose
    z = _odo(cam, "pnp", patch_refine=True, patch_guard=(0, 0))
    zero = _updates(z, pairs)
    for g, w in zip(zero, base):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and not g[4]
    assert z.patch_status == 0 and z.pose_information is None
