"""The dense direct alignment with the affine brightness term on the device (k_direct_align_ab behind vo_direct_align_ab,
csrc/direct.hip) held to its restatement (tests/direct_ab_ref.py) on the planted cases of tests/direct_ab_cases.py, and
StereoOdometer(direct_refine=True, direct_affine=True) on a corridor whose exposure moves from frame to frame.

    matrix         every case of direct_ab_cases.CASES, planted into two dense slots of the test-only library (plant_dense_pair), at the
                   bars of tests/test_gpu_direct.py: status, iterations completed, s, every per-level count and `unknowns` EXACTLY
                   (tests/test_direct_ab_ref.py asserts the decision margin that makes them comparable); the pose within 1e-9; k and m
                   within 1e-9 max(1, |value|); sum w r^2 of every level's first and last iteration and of the last linearisation and
                   the 36 (or 21) sums of H within 1e-9 relative, each to its own magnitude; the 8 (or 6) sums of g within 1e-9 of
                   the sum of their terms' magnitudes (g cancels to zero as the iteration converges: tests/test_gpu_direct.py says why
                   that is its scale).  Every figure is printed before it is asserted; where a plain relative difference exceeds
                   1e-9 the np.longdouble run of the same sums is added and the report says which float64 side is nearer to it.
                   The marginalised information of the binding equals the restatement's to 1e-6 of its largest entry.
    repeatability  the same call twice: a bit-identical record
    affine=False   the record of a plain direct_align call, bit for bit, before and after affine calls on the same context
    misuse         the new errors: iters < 3 (VO_E_ARG from the library, ValueError from the binding), and that the entry shares
                   vo_direct_align's other refusals (a range, a slot without a disparity, two sizes): a refused call writes no record
    the odometer   corridor T0 (320 x 240, D 32), six frames, pose_method="pnp", both images of the ODD frames through
                   rint(0.7 x + 40) before upload: run() equals update() bit for bit, direct_status 0 and direct_brightness set on every
                   accepted frame, k - 1 alternates in sign from pair to pair, the affine chain ends nearer to the ground truth than
                   the unrefined chain of the same process; the plain-refined chain's end point is printed, not asserted.

Measured on one MI355X: over the matrix the pose differs by at most 4.5e-14 (1.2e-11 on `starved_midway`, whose start is 1.2 m off), k
by at most 3.1e-16 and m by 2.1e-14 of max(1, |value|), sum w r^2 by 4.8e-13, the sums of H by 2.0e-13 relative (3.2e-11 on
`starved_midway`), the sums of g by 1.1e-13 of their terms' magnitudes (1.2e-12 on `starved_midway`).  The odometer: gain per pair 1.489 / 0.730 / 1.495 / 0.717 / 1.487; end point
0.3122 m unrefined, 0.1925 m affine-refined, 0.1938 m plain-refined, 3 of 5 refined poses taken in both refined chains.

The planted cases run in ONE child process on the test-only library (VO355_LIB); the cases are the parametrisation."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_ab_cases as AC               # noqa: E402
import direct_ab_ref as AR                 # noqa: E402
import direct_cases as DC                  # noqa: E402

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
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _compare(case, got, want):
    """every figure printed, then asserted"""
    A, B, disp, Q, K4, Rt0, _ = case.build()
    ints = ("status", "iters_done", "s", "selected", "n_first", "n_last", "count", "unknowns")
    nu = int(want["unknowns"])
    nh = nu * (nu + 1) // 2
    d_pose = float(np.abs(got["Rt"] - want["Rt"]).max())
    d_k = abs(got["gain"] - want["gain"]) / max(1.0, abs(want["gain"]))
    d_m = abs(got["offset"] - want["offset"]) / max(1.0, abs(want["offset"]))
    r_wr2 = max(_rel(got["wr2_first"], want["wr2_first"]), _rel(got["wr2_last"], want["wr2_last"]), _rel(got["wr2"], want["wr2"]))
    scale = np.where(want["sums_abs"] > 0, want["sums_abs"], 1.0)
    r_g = float(np.max((np.abs(got["sums"] - want["sums"]) / scale)[nh:nh + nu]))
    plain = np.abs(got["sums"] - want["sums"]) / np.where(np.abs(want["sums"]) > 0, np.abs(want["sums"]), 1.0)
    r_H = float(plain[:nh].max())
    info_scale = float(np.abs(want["information"]).max())
    r_info = float(np.abs(got["information"] - want["information"]).max() / (info_scale if info_scale > 0 else 1.0))
    print("%s: status %d / %d, iterations %d / %d, unknowns %d / %d, s %s, selected %s, first %s, last %s | pose %.2e, k %.12g (%.2e), m %.12g "
          "(%.2e), wr2 %.2e, H %.2e relative, g %.2e of its terms' magnitudes (g plain relative: %.2e), marginalised information %.2e"
          % (case.name, got["status"], want["status"], got["iters_done"], want["iters_done"], got["unknowns"], nu, got["s"].tolist(),
             got["selected"].tolist(), got["n_first"].tolist(), got["n_last"].tolist(), d_pose, got["gain"], d_k, got["offset"], d_m, r_wr2, r_H, r_g,
             float(plain[nh:nh + nu].max()), r_info), flush=True)
    if plain.max() > BAR:                              # the referee: the same sums in extended precision
        ld = AR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, sum_dtype=np.longdouble, **case.kw)
        k = int(np.argmax(plain))
        e_dev, e_ref = abs(got["sums"][k] - ld["sums"][k]), abs(want["sums"][k] - ld["sums"][k])
        print("    sum %d (%s): device %.17g, float64 restatement %.17g, np.longdouble %.17g, magnitudes %.3g: the %s is nearer (%.2e against %.2e)"
              % (k, "H" if k < nh else "g", got["sums"][k], want["sums"][k], ld["sums"][k], want["sums_abs"][k],
                 "device" if e_dev <= e_ref else "restatement", e_dev, e_ref), flush=True)
    for k in ints:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), "%s: %s is %s, the restatement's %s" % (case.name, k, got[k], want[k])
    assert got["status"] == case.expect["status"]
    assert not got["sums"][nh + nu:].any(), "%s: sums past the %d of %d unknowns are not zero" % (case.name, nh + nu, nu)
    assert d_pose <= BAR, "%s: the pose differs by %.3e" % (case.name, d_pose)
    assert d_k <= BAR and d_m <= BAR, "%s: k differs by %.3e, m by %.3e (of max(1, |value|))" % (case.name, d_k, d_m)
    assert r_wr2 <= BAR, "%s: sum w r^2 differs by %.3e relative" % (case.name, r_wr2)
    assert r_H <= BAR, "%s: a sum of H differs by %.3e relative" % (case.name, r_H)
    assert r_g <= BAR, "%s: a sum of g differs by %.3e of its terms' magnitudes" % (case.name, r_g)
    # the Schur complement amplifies the sums' 1e-9 by the conditioning of the brightness block: 1e-6 of the largest entry
    assert got["information_full"].shape == (8, 8) and got["information"].shape == (6, 6) and r_info <= 1e-6, (case.name, r_info)
    return dict(pose=d_pose, wr2=r_wr2, H=r_H, g=r_g)


def _matrix_body():
    out, plain_ctx = {}, _context()
    for case in AC.CASES:
        def check(case=case):
            A, B, disp, Q, K4, Rt0, _ = case.build()
            ctx = plain_ctx if case.roi is None else _context(case.roi)
            ctx.set_Q(Q)
            _plant(ctx, 0, A, disp)
            _plant(ctx, 1, B, disp)
            got = ctx.direct_align(0, 1, K4, Rt0, affine=True, **case.kw)
            again = ctx.direct_align(0, 1, K4, Rt0, affine=True, **case.kw)
            if ctx is not plain_ctx:
                ctx.close()
            want = AR.align(A, B, disp, Q, K4, Rt0, roi=case.roi, **case.kw)
            assert want["margin"] >= AC.MARGIN
            res = _compare(case, got, want)
            assert _same_record(got, again), "%s: the same call twice gave two records" % case.name
            return res
        _run(out, case.name, check)
    plain_ctx.close()
    print("DIRECT-AB-RESULT " + json.dumps(out))


def _misuse_body():
    from openvo_amd import _native
    case = AC.BY_NAME["small_gain"]
    A, B, disp, Q, K4, Rt0, _ = case.build()
    out, ctx = {}, _context()
    ctx.set_Q(Q)
    _plant(ctx, 0, A, disp)
    _plant(ctx, 1, B, disp)
    plain_before = ctx.direct_align(0, 1, K4, Rt0, **case.kw)
    good = ctx.direct_align(0, 1, K4, Rt0, affine=True, **case.kw)
    assert good["status"] == 0 and good["unknowns"] == 8

    def raw(code, slot_a=0, slot_b=1, **over):
        """past the Python layer's own checks: the library's; a refused call writes no record"""
        rec = _native.DirectAbRec()
        prm = dict(case.kw, **over)
        rc = ctx._lib.vo_direct_align_ab(ctx._h, slot_a, slot_b, _native._p(np.float64(K4)), _native._p(np.float64(Rt0).reshape(12)),
                                         prm["levels"], prm["iters"], prm["max_points"], prm["grad_min"], prm["huber"], prm["dmin"], prm["dmax"],
                                         prm["z_min"], prm["min_pixels"], ctypes.byref(rec))
        assert rc == code, "status %d, expected %d (%r)" % (rc, code, over)
        assert rec.levels == 0 and rec.unknowns == 0 and not any(rec.Rt[:]) and rec.k == 0.0, "a refused call wrote its record"

    def iters():
        for n in (0, 1, 2, 21):
            raw(VO_E_ARG, iters=n)
        msg = (ctx._lib.vo_last_error(ctx._h) or b"").decode()
        assert "vo_direct_align_ab" in msg and "3 .. 20" in msg, msg
        for n in (1, 2):
            try:
                ctx.direct_align(0, 1, K4, Rt0, affine=True, **dict(case.kw, iters=n))
            except ValueError as e:
                assert "3 .. 20" in str(e)
            else:
                raise AssertionError("iters=%d with affine=True: not refused" % n)
        assert ctx.direct_align(0, 1, K4, Rt0, **dict(case.kw, iters=2))["status"] == 0      # the plain entry keeps its range
        try:
            ctx.direct_align(0, 1, K4, Rt0, affine=1, **case.kw)
        except ValueError:
            pass
        else:
            raise AssertionError("affine=1: not refused")

    def shared():
        raw(VO_E_ARG, levels=5)
        raw(VO_E_ARG, min_pixels=5)
        raw(VO_E_ARG, slot_a=-1)
        ctx.upload_pair(2, A, A, True)                 # an image pair, no disparity
        raw(VO_E_STATE, slot_a=2)
        raw(VO_E_STATE, slot_b=3)                      # an empty slot
        big = DC.BY_NAME["levels3"].build()
        _plant(ctx, 5, big[1], big[2])                 # another size
        raw(VO_E_STATE, slot_b=5)
        assert _same_record(good, ctx.direct_align(0, 1, K4, Rt0, affine=True, **case.kw))      # the refusals touched nothing

    def plain_unchanged():
        """affine=False is the plain call: the record of before the affine calls, bit for bit, and today's keys"""
        for kw in (dict(), dict(affine=False)):
            r = ctx.direct_align(0, 1, K4, Rt0, **dict(case.kw, **kw))
            assert _same_record(plain_before, r)
        assert set(plain_before) == {"status", "iters_done", "s", "selected", "n_first", "n_last", "wr2_first", "wr2_last", "Rt", "sums",
                                     "information", "g", "count", "wr2"} and plain_before["sums"].shape == (27,)

    for name, fn in (("iters", iters), ("shared", shared), ("plain_unchanged", plain_unchanged)):
        _run(out, name, fn)
    ctx.close()
    print("DIRECT-AB-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ the tests
_RESULTS, _STOPPED = {}, []


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_direct_ab as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIRECT-AB-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("DIRECT-AB-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("DIRECT-AB-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", [c.name for c in AC.CASES])
def test_matches_the_restatement_and_repeats(name):
    res = _child("_matrix_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", ("iters", "shared", "plain_unchanged"))
def test_misuse_and_the_plain_call(name):
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
    table = AC.TABLES["gain"]
    pairs = [(np.ascontiguousarray(table(L)), np.ascontiguousarray(table(R))) if k % 2 else (L, R) for k, (L, R) in enumerate(c.pairs(0, FRAMES))]
    yield dict(ctx=cx, cam=cam, pairs=pairs, gt=c.gt_pose(FRAMES - 1))
    cx.close()


def _odo(cam, **kw):
    from openvo_amd import StereoOdometer
    return StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp", rigidity_threshold=0.1, outlier_threshold=0.02, **kw)


def _state(o, ok):
    return (ok, o.skip_cause, o.c_T_w.copy(), getattr(o, "direct_status", None), getattr(o, "direct_accepted", None), o.direct_brightness)


def _end_error(o, gt):
    return float(np.linalg.norm(np.linalg.inv(o.c_T_w)[:3, 3] - gt[:3, 3]))


def test_odometer_on_a_moving_exposure(rig):
    cam, pairs = rig["cam"], rig["pairs"]
    unrefined = _odo(cam)
    for L, R in pairs:
        unrefined.update(L, R)
    unrefined.reset_lookahead()
    plain = _odo(cam, direct_refine=True)
    plain_taken = 0
    for L, R in pairs:
        plain_taken += bool(plain.update(L, R) and plain.direct_accepted)
    plain.reset_lookahead()
    assert plain.direct_brightness is None and "direct_brightness" not in vars(plain)
    a = _odo(cam, direct_refine=True, direct_affine=True)
    want = []
    for L, R in pairs:
        want.append(_state(a, a.update(L, R)))
    a.reset_lookahead()
    b = _odo(cam, direct_refine=True, direct_affine=True)
    got = [_state(b, ok) for ok in b.run(iter(pairs))]
    b.reset_lookahead()
    assert len(got) == len(want) == FRAMES
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]) and g[3] == w[3] and g[4] == w[4] and g[5] == w[5], k
    gains, taken, accepted, older = {}, 0, 0, 0       # older: the frame the pair of frame k has as its template
    for k, w in enumerate(want[1:], 1):
        if w[0]:
            assert w[3] == 0 and w[5] is not None, (k, w[3], w[5])      # every accepted frame: all iterations ran, a brightness was estimated
            accepted += 1
            taken += bool(w[4])
            gains[(older, k)] = w[5][0]
            older = k
    print("gain per pair (template frame, newer frame) %s" % {p: round(g, 4) for p, g in gains.items()})
    assert accepted >= 3
    # k - 1 alternates in sign: the darker odd frame is B (k > 1) or the template (k < 1); a pair of one parity makes no claim
    mixed = {p: g for p, g in gains.items() if (p[0] + p[1]) % 2}
    assert len(mixed) >= 3 and all((g > 1.0) == (p[1] % 2 == 1) for p, g in mixed.items()), gains
    assert a.pose_information is not None and a.pose_information.shape == (6, 6) and (np.linalg.eigvalsh(a.pose_information) > 0).all()
    assert a.direct_record["unknowns"] == 8 and np.array_equal(a.pose_information, a.direct_record["information"])
    e_un, e_plain, e_ab = _end_error(unrefined, rig["gt"]), _end_error(plain, rig["gt"]), _end_error(a, rig["gt"])
    print("end-point error after %d frames, odd frames through x 0.7 + 40: %.4f m unrefined, %.4f m affine-refined (%d of %d poses taken), "
          "%.4f m plain-refined (%d of %d taken; printed, not asserted)" % (FRAMES, e_un, e_ab, taken, FRAMES - 1, e_plain, plain_taken, FRAMES - 1))
    assert taken >= 1 and e_ab < e_un
