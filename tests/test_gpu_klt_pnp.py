"""The Lucas-Kanade PnP pair step (vo_klt_pnp_pair / _begin / _end: k_klt_track -> k_klt_pnp_prep in csrc/geom.hip -> the tail of the
stereo PnP step) held to the COMPOSED chain on the same device: ctx.klt_track -> the host filter of StereoOdometer._pair_klt ->
ctx.points3d_at (dense) or the planted per-keypoint cloud (sparse) -> ctx.ransac_pnp.  Each link of that chain is already held to a
restatement or to the oracle (tests/test_gpu_klt.py, test_gpu_klt_definitions.py, test_gpu_planted_dense.py, test_gpu_ransac_*).

Planted pairs.  The 160 x 120 smooth pair of tests/klt_cases.py (b = a shifted by (2.5, -1.25) px, a flat rectangle in both) and a
CONSTANT disparity of 8 px in slot a: with Q = (f 120, centre (80, 60), baseline 0.1) every pixel lies at Z = 1.5, a pure image
shift is a pure camera translation of a fronto-parallel plane, and the composed chain finds a real consensus.  A case is admitted
only if the composed chain's best_count >= 0.8 n (the winner is an unrefined minimal-sample pose: a small rotation may stand in for part
of the translation, so the consensus, not the pose, is what says the case is real); the cases with n < 4 have no RANSAC to admit (ctx.ransac_pnp needs four points):
they hold the step to "no pose" -- best (0, 0), Rt all zero, mask 0 -- and the output says so.

Keypoints, in this order (a count N takes the first N): four interior points (so N = 1, 3, 4 sit around the n < 4 decision), the
flat rectangle (status 1), points within `win` of every border of the crop (status 2 where the shift takes them out of the image),
in dense mode two keypoints on a planted 4 x 4 disparity hole (no usable tap: dropped, flag bit 0), in sparse mode two keypoints whose
planted 3-D point holds a NaN / an inf, then random sub-pixel points over the crop.  N = 63 and above hold all of them.

Refit (refine = 3) and LO rounds (lo_rounds = 2): ROUTE TAKEN = the existing planted route.  The compacted arrays of the step are
planted as two sparse slots (plant_keypoints: X as the 3-D points of the first, xy as the positions of the second, one random
descriptor per correspondence in both, so that the ratio test keeps match i -> i in order) and ctx.pnp_pair / pnp_pair_lo on them
runs k_pnp_finish on the same (X, uv): Rt, Rt_refined, refine_status, refine_steps, mask, lo_rounds, lo_support must be equal bit for bit.

One child process per body against the test-only library (planting needs its hooks); the odometer tests run in this process."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_cases as C                      # noqa: E402
import klt_ref as K                        # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
F, CX, CY, INV_B, DISP = 120.0, 80.0, 60.0, 10.0, 8
K4 = (F, F, CX, CY)
Z = F / (INV_B * DISP)
ROI = (9, 5, 152, 114)
COUNTS = (1, 3, 4, 63, 64, 65, 255, 256, 257, 513)
HOLE = (100, 80)                           # x, y of the 4 x 4 disparity hole, image pixels
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
SCALARS = ("matches", "n", "flags", "best_iter", "best_count", "refine_status", "refine_steps", "lo_rounds", "lo_support")


# ------------------------------------------------------------------------------------------------ in the child process
def _context():
    from openvo_amd import _native
    ctx = _native.Context(0, 320, 240, 32, 400)           # kp_cap = 1824
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3], Q[3, 2] = -CX, -CY, F, INV_B
    ctx.set_Q(Q)
    return ctx


def _crop(roi):
    return (0, 0, W, H) if roi is None else roi


def _keypoints(n, roi):
    """the first n planted keypoints in crop pixels -> (xy, indices of the two special-depth keypoints that exist)"""
    x0, y0, x1, y1 = _crop(roi)
    cw, ch = x1 - x0, y1 - y0
    fx, fy, fw, fh = C.flat_rect(W, H)
    sp = [(70.37 - x0, 90.21 - y0), (30.5 - x0, 95.25 - y0), (120.75 - x0, 30.4 - y0), (25.3 - x0, 40.6 - y0),
          (fx + fw / 2.0 + 0.25 - x0, fy + fh / 2.0 - 0.5 - y0), (fx + 10.5 - x0, fy + 12.0 - y0),
          (cw - 0.8, ch * 0.5), (0.3, ch * 0.5 + 3.0), (cw * 0.5, 0.2), (cw * 0.5 + 5.0, ch - 0.7), (cw - 1.9, 1.1), (1.2, ch - 1.4),
          (HOLE[0] + 1.5 - x0, HOLE[1] + 1.5 - y0), (HOLE[0] + 1.25 - x0, HOLE[1] + 2.0 - y0)]
    rng = np.random.default_rng(17)
    rnd = np.stack([rng.uniform(0, cw - 1.001, 600), rng.uniform(0, ch - 1.001, 600)], 1)
    xy = np.concatenate([np.array(sp, np.float64), rnd])[:n].astype(np.float32).reshape(-1, 2)
    assert (xy >= 0).all() and (xy[:, 0] < cw).all() and (xy[:, 1] < ch).all()
    return xy, [i for i in (12, 13) if i < n]


def _disp16():
    d = np.full((H, W), DISP * 16, np.int16)
    d[HOLE[1]:HOLE[1] + 4, HOLE[0]:HOLE[0] + 4] = 0       # reprojects to inf: a tap there is not usable
    return d


def _cloud(xy, roi, special, k4=K4):
    """the per-keypoint 3-D points of the plane (float32) under the camera k4, a NaN and an inf coordinate at the special keypoints"""
    x0, y0 = _crop(roi)[:2]
    X = np.stack([(xy[:, 0].astype(np.float64) + x0 - k4[2]) * Z / k4[0], (xy[:, 1].astype(np.float64) + y0 - k4[3]) * Z / k4[1],
                  np.full(len(xy), Z)], 1).astype(np.float32)
    for k, i in enumerate(special):
        X[i, k] = (np.nan, np.inf)[k]
    return X


def _plant(ctx, slot, img, xy, roi, dense, special, k4=K4):
    if dense:
        ctx.plant_dense_pair(slot, img, _disp16(), xy)
        return None
    ctx.upload_pair(slot, img, img, True)
    X = _cloud(xy, roi, special, k4)
    ctx.plant_keypoints(slot, xy, np.zeros((len(xy), 32), np.uint8), X)
    return X


def _composed(ctx, sa, sb, xy_a, cloud, roi, klt, pnp, k4=K4):
    """the chain StereoOdometer._pair_klt composes, link by link -> the record the fused step must return"""
    xy_b, st, _ = ctx.klt_track(sa, sb, **klt)
    idx = np.nonzero(st == 0)[0]
    flags = 0
    if cloud is None:
        pts, st_a = ctx.points3d_at(sa, xy_a[idx]) if len(idx) else (np.zeros((0, 3), np.float32), np.zeros(0, np.uint8))
        flags = int((st_a == 2).any())
        ok = (st_a == 0) & np.isfinite(pts).all(axis=1)
    else:
        pts = cloud[idx]
        ok = np.isfinite(pts).all(axis=1)
    idx, pts = idx[ok], pts[ok]
    uv = xy_b[idx] + np.array(_crop(roi)[:2], np.float32)
    out = dict(status=st, matches=int((st == 0).sum()), n=len(idx), flags=flags, q=idx.astype(np.int32), xy=xy_b[idx], X=pts, uv=uv)
    if len(idx) >= 4:
        r = ctx.ransac_pnp(pts, uv, k4, pnp["iters"], pnp["thr"], pnp["seed"])
        out.update(best_iter=r["best_iter"], best_count=r["best_count"], mask=r["mask"], Rt=r["Rt"])
    else:
        out.update(best_iter=0, best_count=0, mask=np.zeros(len(idx), np.uint8), Rt=np.zeros((3, 4)))
    return out


def _poison(ctx):
    for a in ctx._klt_pnp_out(True)[1]:
        a[:] = 0x5A


def _full(ctx, r, nq):
    """the record with mask / q as the step wrote them for ALL nq keypoints (the binding cuts them at n)"""
    r = dict(r)
    r["mask_full"], r["q_full"] = ctx._klt_pnp_arrays[0][:nq].copy(), ctx._klt_pnp_arrays[1][:nq].copy()
    return r


def _same_record(a, b, what):
    for k in SCALARS:
        assert a[k] == b[k], "%s: %s %s != %s" % (what, k, a[k], b[k])
    for k in ("Rt", "Rt_refined", "mask", "q", "xy", "mask_full", "q_full"):
        assert C.same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def _hold(r, want, nq, what):
    assert (r["matches"], r["n"], r["flags"]) == (want["matches"], want["n"], want["flags"]), "%s: (M, n, flags) = (%d, %d, %d), composed (%d, %d, %d)" % (
        what, r["matches"], r["n"], r["flags"], want["matches"], want["n"], want["flags"])
    n = want["n"]
    assert np.array_equal(r["q"], want["q"]) and C.same_bits(r["xy"], want["xy"]), "%s: q / xy differ from the composed chain's" % what
    assert (r["q_full"][n:] == -1).all() and not r["mask_full"][n:].any(), "%s: the tails of q / mask" % what
    assert (r["best_iter"], r["best_count"]) == (want["best_iter"], want["best_count"]), "%s: best (%d, %d), composed (%d, %d)" % (
        what, r["best_iter"], r["best_count"], want["best_iter"], want["best_count"])
    if not r["lo_rounds"]:                                  # (behind completed LO rounds the mask is the final set: held to the planted route)
        assert np.array_equal(r["mask"], want["mask"]), "%s: mask differs in %d places" % (what, int((r["mask"] != want["mask"]).sum()))
    assert np.array_equal(r["Rt"], want["Rt"]), "%s: Rt is not that of ransac_pnp on the composed arrays" % what


def _planted_route(ctx, want, roi, pnp, refine, lo_rounds, k4=K4):
    """the refit of ctx.pnp_pair[_lo] on the compacted arrays planted as two sparse slots (slots 6, 7)"""
    n = want["n"]
    desc = np.random.default_rng(5).integers(0, 256, (n, 32)).astype(np.uint8)
    ctx.plant_keypoints(6, np.zeros((n, 2), np.float32), desc, want["X"])
    ctx.plant_keypoints(7, want["xy"], desc, np.ones((n, 3), np.float32))
    kw = dict(iters=pnp["iters"], thr=pnp["thr"], seed=pnp["seed"], refine=refine, want_matches=True)
    r = ctx.pnp_pair_lo(6, 7, 0.8, k4, lo_rounds, **kw) if lo_rounds else ctx.pnp_pair(6, 7, 0.8, k4, **kw)
    assert r["n"] == n and np.array_equal(r["q"], np.arange(n)) and np.array_equal(r["t"], np.arange(n)), "the planted route lost a correspondence"
    return r


CASES = [dict(name="%s_n%d" % (mode, n), n=n, dense=mode == "dense") for mode in ("dense", "sparse") for n in COUNTS] + [
    dict(name="dense_roi_n257", n=257, dense=True, roi=ROI), dict(name="sparse_roi_n257", n=257, dense=False, roi=ROI),
    dict(name="dense_fb0_n257", n=257, dense=True, fb=0.0), dict(name="dense_win9_levels2_n257", n=257, dense=True, win=9, levels=2),
    dict(name="sparse_win9_levels2_n65", n=65, dense=False, win=9, levels=2),
    dict(name="dense_refine3_n257", n=257, dense=True, refine=3), dict(name="sparse_refine3_roi_n513", n=513, dense=False, refine=3, roi=ROI),
    dict(name="dense_lo2_n257", n=257, dense=True, refine=3, lo_rounds=2)]
CASE_NAMES = [c["name"] for c in CASES]


def _check_case(ctx, a, b, c):
    roi, dense, n = c.get("roi"), c["dense"], c["n"]
    k4 = c.get("K4", K4)                                    # (a sparse case may bring its own camera: its cloud is planted under it)
    klt = dict(win=c.get("win", 21), levels=c.get("levels", 3), fb=c.get("fb", 1.0))
    pnp = dict(iters=256, thr=1.5, seed=4321)
    refine, lo = c.get("refine", 0), c.get("lo_rounds", 0)
    ctx.set_roi(*(roi if roi is not None else (0, 0, 320, 240)))
    try:
        xy, special = _keypoints(n, roi)
        cloud = _plant(ctx, 0, a, xy, roi, dense, special, k4)
        ctx.upload_pair(1, b, b, True)
        want = _composed(ctx, 0, 1, xy, cloud, roi, klt, pnp, k4)
        st = want["status"]
        line = "%s: N %d  status 0 / 1 / 2 / 8: %d / %d / %d / %d  composed (M, n, flags) = (%d, %d, %d) best %d @ %d" % (
            c["name"], n, (st == 0).sum(), (st & 1).astype(bool).sum(), (st & 2).astype(bool).sum(), (st & 8).astype(bool).sum(),
            want["matches"], want["n"], want["flags"], want["best_count"], want["best_iter"])
        if want["n"] < 4:
            print(line + "  -- n < 4: no RANSAC to admit, held to the no-pose record", flush=True)
        else:
            print(line, flush=True)
            assert want["best_count"] >= 0.8 * want["n"], "NOT ADMITTED: the composed chain's consensus is %d of %d" % (want["best_count"], want["n"])
        if n >= 63:                                         # the planted properties of the case
            assert (st & 1).any() and (st == 0).sum() >= 30, "no flat-rectangle point / too few tracks"
            if roi is None:
                assert (st & 2).any(), "no track left the image"
            assert want["n"] < want["matches"], "no track was dropped by the 3-D lookup"
            assert want["flags"] == (1 if dense else 0)
        kw = dict(refine=refine, lo_rounds=lo, want_arrays=True, **pnp, **klt)
        _poison(ctx)
        r = _full(ctx, ctx.klt_pnp_pair(0, 1, k4, **kw), n)
        _hold(r, want, n, "klt_pnp_pair")
        tk = ctx.klt_pnp_pair_begin(0, 1, k4, **kw)
        _poison(ctx)
        r2 = _full(ctx, ctx.klt_pnp_pair_end(tk, want_arrays=True), n)
        _same_record(r, r2, "klt_pnp_pair and klt_pnp_pair_begin / _end")
        bare = ctx.klt_pnp_pair(0, 1, k4, **dict(kw, want_arrays=False))
        assert all(bare[k] == r[k] for k in SCALARS) and np.array_equal(bare["Rt"], r["Rt"]) and "xy" not in bare
        if refine:
            assert want["n"] >= 6
            ref = _planted_route(ctx, want, roi, pnp, refine, lo, k4)
            keys = ("refine_status", "refine_steps", "best_iter", "best_count") + (("lo_rounds", "lo_support") if lo else ())
            for k in keys:
                assert r[k] == ref[k], "%s: %s, the planted route %s" % (k, r[k], ref[k])
            assert r["refine_status"] == 0 and r["refine_steps"] == refine * max(lo, 1)
            assert np.array_equal(r["Rt"], ref["Rt"]) and np.array_equal(r["Rt_refined"], ref["Rt_refined"]), "Rt_refined is not the planted route's"
            assert np.array_equal(r["mask"], ref["mask"])
            assert not np.array_equal(r["Rt_refined"], r["Rt"])
            print("    refit by the planted route: status %d, %d steps, |Rt_refined - Rt| = %.3g" % (
                r["refine_status"], r["refine_steps"], float(np.abs(r["Rt_refined"] - r["Rt"]).max())), flush=True)
        else:
            assert r["refine_status"] == 1 and np.array_equal(r["Rt_refined"], r["Rt"]) and (r["lo_rounds"], r["lo_support"]) == (0, r["best_count"])
    finally:
        ctx.set_roi(0, 0, 320, 240)


def _planted_body():
    ctx = _context()
    a, b = C.smooth_pair(W, H)
    out = {}
    for c in CASES:
        try:
            _check_case(ctx, a, b, c)
            out[c["name"]] = dict(ok=True)
        except AssertionError as e:                        # (anything else -- a native error status, a fault -- ends the child)
            out[c["name"]] = dict(ok=False, err=str(e)[:1500])
            print("%s: FAILED %s" % (c["name"], out[c["name"]]["err"]), flush=True)
    # zero keypoints through the C entry: the cleared record, nothing launched
    ctx.plant_dense_pair(0, a, _disp16(), np.zeros((0, 2), np.float32))
    try:
        r = ctx.klt_pnp_pair(0, 1, K4, want_arrays=True)
        tk = ctx.klt_pnp_pair_begin(0, 1, K4, want_arrays=True)
        r2 = ctx.klt_pnp_pair_end(tk, want_arrays=True)
        for q in (r, r2):
            assert (q["matches"], q["n"], q["flags"], q["best_iter"], q["best_count"], q["refine_status"]) == (0, 0, 0, 0, 0, 1)
            assert not q["Rt"].any() and not q["Rt_refined"].any() and len(q["q"]) == 0 and len(q["xy"]) == 0
        out["zero_keypoints"] = dict(ok=True)
    except AssertionError as e:
        out["zero_keypoints"] = dict(ok=False, err=str(e)[:1500])
    ctx.close()
    print("KLTPNP-RESULT " + json.dumps(out))


HALVES = ("reverse_order", "refill_behind_begin", "orb_and_klt_tickets")


def _halves_body():
    ctx = _context()
    a, b = C.smooth_pair(W, H)
    c = K.smooth_texture(W, H, (5.0, -2.5), seed=C.SMOOTH_SEED)
    xy, _ = _keypoints(257, None)
    kw = dict(iters=256, thr=1.5, seed=4321, refine=3, want_arrays=True, win=21, levels=3, fb=1.0)
    ctx.plant_dense_pair(0, a, _disp16(), xy)
    ctx.plant_dense_pair(1, b, _disp16(), xy[::-1].copy())
    ctx.upload_pair(2, c, c, True)
    out = {}

    def sync(sa, sb):
        _poison(ctx)
        return _full(ctx, ctx.klt_pnp_pair(sa, sb, K4, **kw), 257)

    def end(tk):
        _poison(ctx)
        return _full(ctx, ctx.klt_pnp_pair_end(tk, want_arrays=True), 257)

    def attempt(name, fn):
        try:
            fn()
            out[name] = dict(ok=True)
        except AssertionError as e:
            out[name] = dict(ok=False, err=str(e)[:1500])
            print("%s: FAILED %s" % (name, out[name]["err"]), flush=True)

    want_ab, want_bc = sync(0, 1), sync(1, 2)
    assert want_ab["best_count"] >= 0.8 * want_ab["n"] >= 40 and want_bc["best_count"] >= 0.8 * want_bc["n"] >= 40

    def reverse_order():
        t1, t2 = ctx.klt_pnp_pair_begin(0, 1, K4, **kw), ctx.klt_pnp_pair_begin(1, 2, K4, **kw)
        assert t1 != t2
        got_bc, got_ab = end(t2), end(t1)
        _same_record(got_ab, want_ab, "(a, b) ended last")
        _same_record(got_bc, want_bc, "(b, c) ended first")
        assert not C.same_bits(got_ab["Rt"], got_bc["Rt"])

    def refill_behind_begin():
        tk = ctx.klt_pnp_pair_begin(0, 1, K4, **kw)
        ctx.upload_pair(1, c[::-1].copy(), c[::-1].copy(), True)          # other images into slot b: ordered behind the step's reads
        _same_record(end(tk), want_ab, "slot b refilled behind _begin")
        ctx.plant_dense_pair(1, b, _disp16(), xy[::-1].copy())
        _same_record(sync(0, 1), want_ab, "slot b planted again")

    def orb_and_klt_tickets():
        n = 200
        rng = np.random.default_rng(9)
        desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        X = _cloud(xy[20:20 + n], None, ())
        ctx.plant_keypoints(4, xy[20:20 + n], desc, X)
        ctx.plant_keypoints(5, xy[20:20 + n] + np.array([2.5, -1.25], np.float32), desc, X)
        okw = dict(iters=256, thr=1.5, seed=4321, refine=3, want_matches=True)
        want_orb = ctx.pnp_pair(4, 5, 0.8, K4, **okw)
        assert want_orb["n"] == n and want_orb["best_count"] >= 0.8 * n
        t_orb = ctx.pnp_pair_begin(4, 5, 0.8, K4, **okw)
        t_klt = ctx.klt_pnp_pair_begin(0, 1, K4, **kw)
        assert t_orb != t_klt
        got_klt = end(t_klt)
        got_orb = ctx.pnp_pair_end(t_orb, want_matches=True)
        _same_record(got_klt, want_ab, "the Lucas-Kanade ticket beside a descriptor ticket")
        for k in ("matches", "n", "best_iter", "best_count", "refine_status", "refine_steps"):
            assert got_orb[k] == want_orb[k], k
        for k in ("Rt", "Rt_refined", "mask", "q", "t"):
            assert np.array_equal(got_orb[k], want_orb[k]), k

    attempt("reverse_order", reverse_order)
    attempt("refill_behind_begin", refill_behind_begin)
    attempt("orb_and_klt_tickets", orb_and_klt_tickets)
    ctx.close()
    print("KLTPNP-RESULT " + json.dumps(out))


def _refusals_body():
    """every refusal leaves the outputs untouched (and a refused ticket open)"""
    from openvo_amd import _native
    ctx = _context()
    lib, hd, p = ctx._lib, ctx._h, _native._p
    a, b = C.smooth_pair(W, H)
    xy, _ = _keypoints(65, None)
    cap = ctx.kp_cap
    K4a = np.array(K4, np.float64)
    outs = None

    def fresh():
        return [np.full(4, -7, np.int32), np.full(1, -7, np.int32), np.full(12, -7.0), np.full(12, -7.0), np.full(2, -7, np.int32),
                np.full(2, -7, np.int32), np.full(cap, 0xEE, np.uint8), np.full(cap, -7, np.int32), np.full((cap, 2), -7.0, np.float32)]

    def untouched():
        return all((o == v).all() for o, v in zip(outs, (-7, -7, -7.0, -7.0, -7, -7, 0xEE, -7, -7.0)))

    def call(sa=0, sb=1, win=21, levels=3, kit=30, fb=1.0, K=K4a, iters=256, thr=1.5, refine=0, lo=0, cap_=cap, handle=hd, drop=()):
        nonlocal outs
        outs = fresh()
        args = [None if i in drop else p(o) for i, o in enumerate(outs)]
        rc = lib.vo_klt_pnp_pair(handle, sa, sb, win, levels, kit, 0.01, 1e-4, fb, None if K is None else p(K), iters, thr, 4321, refine, lo, *args, cap_)
        assert rc == 0 or untouched(), "a refused call wrote an output"
        return rc

    def begin(sa=0, sb=1, win=21, levels=3, iters=256, thr=1.5, refine=0, lo=0, ticket=True):
        t = ctypes.c_int(-5)
        rc = lib.vo_klt_pnp_pair_begin(hd, sa, sb, win, levels, 30, 0.01, 1e-4, 1.0, p(K4a), iters, thr, 4321, refine, lo, 1, ctypes.byref(t) if ticket else None)
        assert rc == 0 or t.value == -5
        return rc, t.value

    out = {}
    try:
        ctx.upload_pair(0, a, a, True)
        ctx.upload_pair(1, b, b, True)
        assert call() == VO_E_STATE and begin()[0] == VO_E_STATE                     # no keypoints in slot a
        ctx.plant_dense_pair(0, a, _disp16(), xy)
        assert call() == 0 and outs[0][0] > 30
        assert call(sa=-1) == VO_E_ARG and call(sb=_native.VO_NUM_SLOTS) == VO_E_ARG and call(sa=_native.VO_NUM_SLOTS) == VO_E_ARG   # bad slots
        assert call(sb=3) == VO_E_STATE                                              # no pair in slot b
        ctx.upload_pair(3, b[:-8], b[:-8], True)
        assert call(sb=3) == VO_E_STATE and begin(sb=3)[0] == VO_E_STATE             # shapes differ
        ctx.upload_pair(2, a, a, True)
        ctx.orb_slot(2, 200, 0)
        assert call(sa=2) == VO_E_STATE and begin(sa=2)[0] == VO_E_STATE             # a dense slot a without disparity
        for kw in (dict(win=22), dict(win=33), dict(levels=0), dict(levels=7), dict(kit=0), dict(fb=-1.0), dict(iters=0), dict(thr=0.0),
                   dict(refine=21), dict(refine=-1), dict(lo=1), dict(lo=9, refine=3), dict(K=None), dict(K=np.array([0.0, F, CX, CY])),
                   dict(drop=(0,)), dict(drop=(1,)), dict(drop=(2,)), dict(drop=(4,)), dict(handle=None)):
            assert call(**kw) == VO_E_ARG, kw
        for kw in (dict(win=22), dict(levels=0), dict(iters=0), dict(thr=0.0), dict(lo=1), dict(ticket=False)):
            assert begin(**kw)[0] == VO_E_ARG, kw
        assert call(cap_=64) == VO_E_CAP and call(cap_=65) == 0                      # cap too small (65 keypoints)
        assert call(cap_=0, drop=(6, 7, 8)) == 0 and call(drop=(3, 5)) == 0          # no array asked for; Rt12_refined and lo2 are optional
        # tickets ended by the wrong _end, both ways: refused with VO_E_STATE, and the ticket stays open for its own _end
        rc, tk = begin()
        assert rc == 0
        o = fresh()
        outs = o
        assert lib.vo_pnp_pair_end(hd, tk, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[6]), p(o[7]), p(o[7]), cap) == VO_E_STATE and untouched()
        lo2 = np.full(2, -7, np.int32)
        assert lib.vo_pnp_pair_end_lo(hd, tk, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[6]), p(o[7]), p(o[7]), cap, p(lo2)) == VO_E_STATE and untouched()
        rc2, T = np.full(2, -7, np.int32), np.full(12, -7.0)
        assert lib.vo_pose_pair_end(hd, tk, p(o[0]), p(rc2), p(T), p(o[2])) == VO_E_STATE and untouched() and (rc2 == -7).all() and (T == -7.0).all()
        assert lib.vo_klt_pnp_pair_end(hd, tk, *[p(v) for v in o], 64) == VO_E_CAP and untouched()
        assert lib.vo_klt_pnp_pair_end(hd, tk, *[p(v) for v in o], cap) == 0 and o[0][0] > 30
        assert lib.vo_klt_pnp_pair_end(hd, tk, *[p(v) for v in o], cap) == VO_E_STATE          # not open any more
        n = 60
        desc = np.random.default_rng(9).integers(0, 256, (n, 32)).astype(np.uint8)
        ctx.plant_keypoints(4, xy[:n], desc, _cloud(xy[:n], None, ()))
        ctx.plant_keypoints(5, xy[:n] + np.array([2.5, -1.25], np.float32), desc, _cloud(xy[:n], None, ()))
        tk = ctx.pnp_pair_begin(4, 5, 0.8, K4)
        o = fresh()
        outs = o
        assert lib.vo_klt_pnp_pair_end(hd, tk, *[p(v) for v in o], cap) == VO_E_STATE and untouched()
        assert ctx.pnp_pair_end(tk)["matches"] == n
        tk = ctx.pose_pair_begin(4, 5, 0.8, 10, 0.0, 0.0)
        assert lib.vo_klt_pnp_pair_end(hd, tk, *[p(v) for v in o], cap) == VO_E_STATE and untouched()
        ctx.pose_pair_end(tk)
        # and the context still works
        assert call() == 0 and outs[0][0] > 30
        out["refusals"] = dict(ok=True)
    except AssertionError as e:
        import traceback
        out["refusals"] = dict(ok=False, err=traceback.format_exc()[-1500:])
    ctx.close()
    print("KLTPNP-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_klt_pnp as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("KLTPNP-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("KLTPNP-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("KLTPNP-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", CASE_NAMES + ["zero_keypoints"])
def test_planted_pair_equals_the_composed_chain(name):
    res = _child("_planted_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", HALVES)
def test_halves(name):
    res = _child("_halves_body()")[name]
    assert res["ok"], res["err"]


def test_refusals_leave_the_outputs_untouched():
    res = _child("_refusals_body()")["refusals"]
    assert res["ok"], res["err"]


# ---- the odometer ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """corridor C1 at 640 x 480, D 64, 500 features: the 12 pairs of the composed-path odometer test"""
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    cx = _native.Context(0, 640, 480, 64, 500)
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=cx)
    yield dict(ctx=cx, cam=cam, pairs=c.pairs(0, 12))
    cx.close()


def _odo(cam, **kw):
    from openvo_amd import StereoOdometer
    return StereoOdometer(cam, preprocessed_frames=True, match="klt", pose_method="pnp", **kw)


@pytest.mark.parametrize("depth,frames", (("dense", 12), ("sparse", 8)))
def test_fused_odometer_equals_the_composed_one_frame_by_frame(rig, depth, frames):
    cam = rig["cam"]
    plain, fused = _odo(cam, depth=depth), _odo(cam, depth=depth, klt_fused=True)
    calls = []
    orig = rig["ctx"].klt_pnp_pair
    rig["ctx"].klt_pnp_pair = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]       # (not a seam of the fused step: it IS the step)
    try:
        for k, (L, R) in enumerate(rig["pairs"][:frames]):
            want, got = plain.update(L, R), fused.update(L, R)
            assert got == want and fused.skip_cause == plain.skip_cause and fused.skipped_frames == plain.skipped_frames, k
            assert fused.klt_counts == plain.klt_counts, (k, fused.klt_counts, plain.klt_counts)
            assert np.array_equal(fused.c_T_w, plain.c_T_w), k
            print("%s frame %2d: accepted %s cause %r tracks %s" % (depth, k, got, fused.skip_cause, fused.klt_counts))
    finally:
        del rig["ctx"].klt_pnp_pair
        fused.reset_lookahead()
        plain.reset_lookahead()
    assert len(calls) + fused.klt_ahead >= frames - 1 and fused.klt_counts[1] >= 100      # (the fused step ran for every pair)
    assert np.linalg.norm(fused.c_T_w[:3, 3]) > 1.0


def test_run_with_steps_begun_ahead_equals_update(rig):
    cam, pairs = rig["cam"], rig["pairs"][:9]
    a = _odo(cam, klt_fused=True)
    want = [(a.update(L, R), a.skip_cause, a.klt_counts, a.c_T_w.copy()) for L, R in pairs]
    a.reset_lookahead()
    b = _odo(cam, klt_fused=True)
    got = [(ok, b.skip_cause, b.klt_counts, b.c_T_w.copy()) for ok in b.run(iter(pairs))]
    assert len(got) == len(want) == 9
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2] and np.array_equal(g[3], w[3])
    print("run(): %d of 8 pair steps collected from a ticket begun ahead" % b.klt_ahead)
    assert b.klt_ahead >= 1
    b.reset_lookahead()
    assert not b._specs


def test_an_orb_odometer_is_unchanged_by_a_fused_klt_odometer_on_the_same_context(rig):
    from openvo_amd import StereoOdometer
    cam, pairs = rig["cam"], rig["pairs"][:5]

    def orb_poses():
        o = StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp")
        out = [(o.update(L, R), o.skip_cause, o.c_T_w.copy()) for L, R in pairs]
        o.reset_lookahead()
        return out

    before = orb_poses()
    k = _odo(cam, klt_fused=True)
    used = list(k.run(iter(pairs)))
    k.reset_lookahead()
    assert used[0] and any(used[1:]) and k.klt_counts[1] >= 100
    after = orb_poses()
    assert all(b[0] for b in before)
    for b, a in zip(before, after):
        assert b[0] == a[0] and b[1] == a[1] and np.array_equal(b[2], a[2])


def test_constructor_refusals(rig):
    from openvo_amd import StereoOdometer
    for kw in (dict(match="orb"), dict(match="klt", pose_method="umeyama")):
        with pytest.raises(ValueError, match="klt_fused"):
            StereoOdometer(rig["cam"], preprocessed_frames=True, klt_fused=True, **kw)
