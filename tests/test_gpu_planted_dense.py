"""The dense depth lookup (bilinear_one over TapDisp, reproject_px under it: csrc/geom.hip) driven through PLANTED disparity images:
vo_test_plant_dense of the test-only library writes an int16 disparity and keypoints into a slot, which then stands as sgbm_compute
+ ORB leave it, so holes, the invalid value, W == 0, the crop edges and the (M, n) of the fused steps are chosen, not what SGBM
and ORB find in the corridor.  Inputs, the numpy restatement and the cases are tests/planted_dense.py; tests/test_planted_dense_ref.py
asserts, without a GPU, that the restatement equals the CPU oracle bit for bit and that every case reaches the regime its name promises.

    points3d_at        k_points3d on every field x Q x ROI, every position set and n = 1, 63, 64, 65, 300 (64-thread blocks): status exact,
                       xyz equal to the oracle in its bits wherever status != 2;  a position with (int)x == cw is refused
    downloads          k_reproject_disp16 / k_disp_to_f32 at 67 x 33 and 300 x 21 (row tails, two 256-wide blocks per row), inf included
    point_clouds       dense slots, nq = 1, 64, 65, 513 (the last: the 1024-thread k_ratio_compact), with and without cross-check
    pose_pair          + pose_pair_begin / _end: held to planted.Case.model fed with the looked-up points, and DIFFERENTIALLY to the same
                       case with both slots sparse-planted with those points: every field bit-identical except flag bit 0, which is set
                       exactly when a matched keypoint has status 2.  k_pose_solve reads neither st_a nor st_b -- only the flag word
                       k_pose_prep derived from them -- so the differential check excludes nothing but that bit.
    pnp_pair           + pnp_pair_begin / _end, slot a dense: (M, n, flags), q / t = the status-0 filter of the numpy matches in match
                       order, uv == xy_b[t] + float32 origin in its bits, the tails of mask / q / t, Rt within BAR_RT of
                       oracle.ransac_pnp and bit-identical with the sparse-planted twin
    the hook           its refusals leave the slot as it was (a points3d_at before and after)

NaN.  Where the definition yields a NaN (status 1: 0 / 0) the comparison is "NaN on both sides": the sign bit of a generated NaN is the
platform's (x86 sets it, the GPU does not), every other value is compared as its bit pattern.

pnp_pair with slot a dense and slot b SPARSE-planted is refused with VO_E_STATE, like point_clouds and pose_pair (pnp_check: "one
slot's keypoints carry depth, the other's do not") although only a's depth would be read; asserted here as the library's contract.
Flag bit 0 at the odometer's level (ZeroDivisionError) needs a StereoCamera around the context and real frames; no seam reaches it
from a planted slot, so the flag alone is asserted.

One child process per group of cases, VO355_LIB pointing at the test-only library; the cases are the parametrisation."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted as P                        # noqa: E402
import planted_dense as D                  # noqa: E402
import planted_pnp as PP                   # noqa: E402
import window_match_ref as WM              # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
BAR_RT = 1e-10                             # the bar tests/test_gpu_planted_pnp.py and tests/test_gpu_pnp_pair.py hold this pose to
SIZES = (1, 63, 64, 65, 300)
DOWNLOAD_SIZES = ((67, 33), (300, 21))
CLOUDS = ((1, 1, 0), (64, 50, 6), (65, 50, 6), (513, 400, 40))        # (nq, M, duplicates the cross-check must remove)
CLOUD_FIELDS = (("hole_blocks", "plain"), ("w_zero", "w33"))


# ------------------------------------------------------------------------------------------------ in the child process
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _roi4(roi):
    return (0, 0, 1 << 20, 1 << 20) if roi is None else roi


def _same_lookup(got, st, want, wst, what):
    assert np.array_equal(st, wst), "%s: status differs in %d places" % (what, int((st != wst).sum()))
    k = wst != 2
    nan = np.isnan(want[k])
    assert np.array_equal(np.isnan(got[k]), nan), "%s: NaN masks differ" % (what,)
    bad = _bits(got[k])[~nan] != _bits(want[k])[~nan]
    assert not bad.any(), "%s: %d values differ from the oracle in their bits" % (what, int(bad.sum()))
    assert np.isnan(got[~k]).all(), "%s: status 2 without a NaN triple" % (what,)


def _same_image(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN masks differ" % (what,)
    bad = _bits(got)[~nan] != _bits(want)[~nan]
    assert not bad.any(), "%s: %d values differ in their bits" % (what, int(bad.sum()))


def _context(roiname, w=D.W, h=D.H):
    from openvo_amd import _native
    ctx = _native.Context(0, w, h, 16, 1024)           # kp_cap = 3072
    if D.ROIS[roiname] is not None:
        ctx.set_roi(*D.ROIS[roiname])                  # (before anything is planted, and never changed afterwards)
    return ctx


def _one_kp():
    return np.float32([[1, 1]]), np.zeros((1, 32), np.uint8)


def _run(out, name, fn):
    try:
        out[name] = dict(ok=True, **(fn() or {}))
    except AssertionError as e:                        # (anything else -- a native error status, a fault -- ends the child)
        out[name] = dict(ok=False, err=str(e)[:1500])
        print("%s: FAILED %s" % (name, out[name]["err"]), flush=True)


def _lookup_body(roiname):
    from openvo_amd import _native
    from oracle import oracle as O
    ctx, roi = _context(roiname), D.ROIS[roiname]
    x0, y0, x1, y1 = D.crop(roi, D.W, D.H)
    out = {}
    for field in D.FIELDS:
        for qname, Q in D.QS.items():
            def check():
                disp = D.FIELDS[field]()
                ctx.set_Q(Q)
                ctx.plant_dense(0, disp, *_one_kp())
                n_all, seen = 0, np.zeros(3, np.int64)
                sets = [(s, D.positions(s, disp, Q, roi)) for s in D.POSITIONS] + [(n, D.mixed_positions(disp, Q, roi, n)) for n in SIZES]
                for s, xy in sets:
                    got, st = ctx.points3d_at(0, xy)
                    want, wst = O.points3d_at(disp, Q, _roi4(roi), xy)
                    _same_lookup(got, st, want, wst, (field, qname, roiname, s))
                    n_all += len(xy)
                    seen += np.bincount(wst, minlength=3)
                # (int)x == cw, (int)y == ch, and what no int holds (the cast of 3e9 or inf is negative: below every cw): refused on the host
                for xy in ([[x1 - x0, 1]], [[1, y1 - y0]], [[x1 - x0 - 1, 1], [x1 - x0, 1]], [[3e9, 1]], [[1, np.inf]], [[np.nan, 1]], [[-0.5, 1]]):
                    with pytest.raises(_native.VoError) as e:
                        ctx.points3d_at(0, np.float32(xy))
                    assert e.value.code == VO_E_ARG, e.value
                print("%s %s %s: %d lookups, status 0 / 1 / 2: %s" % (field, qname, roiname, n_all, seen.tolist()), flush=True)
                return dict(n=n_all, status=seen.tolist())
            _run(out, "%s-%s" % (field, qname), check)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _download_body():
    from oracle import oracle as O
    ctx = _context("none", 304, 64)
    out = {}
    for w, h in DOWNLOAD_SIZES:
        def check():
            n_inf = 0
            for field in D.FIELDS:
                disp = D.FIELDS[field](w, h)
                for qname, Q in D.QS.items():
                    ctx.set_Q(Q)
                    ctx.plant_dense(0, disp, *_one_kp())
                    want = O.reproject_to_3d(disp.astype(np.float32) / np.float32(16.0), Q)
                    _same_image(ctx.download_xyz(0, (h, w)), want, (field, qname, w, h, "xyz"))
                    _same_image(ctx.download_disparity_f32(0, (h, w)), disp.astype(np.float32) / np.float32(16.0), (field, qname, w, h, "disparity"))
                    n_inf += int(np.isinf(want).sum())
            assert n_inf > 0
            return dict(inf=n_inf)
        _run(out, "%dx%d" % (w, h), check)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _want_matches(c, cross):
    if not cross:
        return P.matches(c.dq, c.dt)
    idx, dist, mutual, _ = WM.window_knn2_mutual(c.dq, c.dt, c.xy_a, c.xy_b, 1e9, 1e9)
    q, t = WM.ratio_filter(idx, dist, P.RATIO)
    return q[mutual[q] > 0], t[mutual[q] > 0]


def _clouds_body():
    from openvo_amd import _native
    from oracle import oracle as O
    roiname = "inner"
    ctx, roi = _context(roiname), D.ROIS[roiname]
    out = {}
    for nq, M, dup in CLOUDS:
        for field, qname in CLOUD_FIELDS:
            def check():
                c = PP.PnpCase("clouds", nq, M, dup=dup).build()              # (descriptors with duplicates: the parent's)
                Q, da, db = D.QS[qname], D.FIELDS[field](), D.FIELDS["invalid"]()
                c.xy_a, c.xy_b = D.mixed_positions(da, Q, roi, nq, seed=2), D.mixed_positions(db, Q, roi, len(c.dt), seed=3)
                ctx.set_Q(Q)
                ctx.plant_dense(0, da, c.xy_a, c.dq)
                ctx.plant_dense(1, db, c.xy_b, c.dt)
                fig = {}
                for cross in (False, True):
                    wq, wt = _want_matches(c, cross)
                    q, t, pa, pb, sa, sb = ctx.point_clouds(0, 1, P.RATIO, cross_check=cross)
                    assert np.array_equal(q, wq) and np.array_equal(t, wt), "matches differ from the numpy matcher (cross-check %s)" % cross
                    _same_lookup(pa, sa, *O.points3d_at(da, Q, _roi4(roi), c.xy_a[wq]), (nq, field, "a", cross))
                    _same_lookup(pb, sb, *O.points3d_at(db, Q, _roi4(roi), c.xy_b[wt]), (nq, field, "b", cross))
                    fig["cross" if cross else "plain"] = len(q)
                assert fig["plain"] == M and fig["cross"] == M - dup, "the construction gave %s matches" % (fig,)
                print("nq %d %s: %d matches, %d with the cross-check" % (nq, field, fig["plain"], fig["cross"]), flush=True)
                return fig
            _run(out, "nq%d-%s" % (nq, field), check)

    def mixed():
        """one dense and one sparse-planted slot: VO_E_STATE from every pair step, and both slots remain usable"""
        c = next(c for c in D.POSE_CASES if c.name == "roi_origin_3_5").build()        # (built for the ROI this context has)
        ctx.set_Q(c.Q)
        ctx.plant_dense(0, c.disp_a, c.xy_a, c.dq)
        ctx.plant_keypoints(1, c.xy_b, c.dt, c.xyz_b)
        for call in (lambda: ctx.point_clouds(0, 1, P.RATIO), lambda: ctx.pose_pair(0, 1, P.RATIO, 10, P.RIGIDITY, P.OUTLIER),
                     lambda: ctx.pnp_pair(0, 1, P.RATIO, D.K4S["plain"], 64), lambda: ctx.pnp_pair(1, 0, P.RATIO, D.K4S["plain"], 64)):
            with pytest.raises(_native.VoError) as e:
                call()
            assert e.value.code == VO_E_STATE, e.value
        _same_lookup(*ctx.points3d_at(0, c.xy_a), *O.points3d_at(c.disp_a, c.Q, _roi4(c.roi), c.xy_a), "the dense slot after the refusals")
        xyz, _ = ctx.download_keypoint_depth(1)
        assert np.array_equal(_bits(xyz), _bits(c.xyz_b)), "the sparse slot after the refusals"
        ctx.plant_keypoints(0, c.xy_a, c.dq, c.xyz_a)
        assert len(ctx.point_clouds(0, 1, P.RATIO)[0]) == c.M
    _run(out, "dense_and_sparse", mixed)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _same_T(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _pose_body(roiname):
    import tests.test_gpu_planted_pose as TPose
    from oracle import oracle as O
    ctx = _context(roiname)
    out = {}
    for c in [c for c in D.POSE_CASES if c.roiname == roiname]:
        def check():
            c.build()
            m = c.model(O)
            ctx.set_Q(c.Q)
            fig = TPose._check_case(ctx, O, c)             # the sparse-planted twin (its points: the lookup of EVERY keypoint), held to the model
            args = (0, 1, P.RATIO, c.min_matches, c.rigidity, c.outlier)
            twin = ctx.pose_pair(*args)
            ctx.plant_dense(0, c.disp_a, c.xy_a, c.dq)
            ctx.plant_dense(1, c.disp_b, c.xy_b, c.dt)
            q, t, pa, pb, sa, sb = ctx.point_clouds(0, 1, P.RATIO)
            assert np.array_equal(q, m["q"]) and np.array_equal(t, m["t"]), "matches differ from the numpy brute force"
            _same_lookup(pa, sa, *O.points3d_at(c.disp_a, c.Q, _roi4(c.roi), c.xy_a[q]), "slot a")
            _same_lookup(pb, sb, *O.points3d_at(c.disp_b, c.Q, _roi4(c.roi), c.xy_b[t]), "slot b")
            want_flags = c.dense_flags(m)
            bit0 = int((sa == 2).any() or (sb == 2).any())
            assert bit0 == (want_flags & 1)
            for how, (counts, rc, T1, T2) in (("pose_pair", ctx.pose_pair(*args)), ("pose_pair_begin / _end", ctx.pose_pair_end(ctx.pose_pair_begin(*args)))):
                print("%s %s: counts %s rc %s, the twin's %s %s, the model's %s + bit 0 = %d" % (c.name, how, counts, rc, twin[0], twin[1], m["counts"], bit0), flush=True)
                assert tuple(int(v) for v in counts[:3]) == m["counts"][:3] and tuple(int(v) for v in rc) == m["rc"], "%s: counts / rc differ from the model" % how
                assert int(counts[3]) == want_flags, "%s: flags %d, want %d" % (how, counts[3], want_flags)
                assert np.array_equal(counts[:3], twin[0][:3]) and int(counts[3]) & ~1 == int(twin[0][3]) and np.array_equal(rc, twin[1]), "%s: differs from the sparse-planted twin" % how
                for k, got, want, code in (("T1", T1, twin[2], rc[0]), ("T2", T2, twin[3], rc[1])):
                    if code == 0:
                        assert _same_T(got, want), "%s: %s is not bit-identical with the sparse-planted twin (max diff %.3g)" % (how, k, float(np.nanmax(np.abs(got - want))))
            fig["flags"] = want_flags
            return fig
        _run(out, c.name, check)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


PNP_SCALARS = ("matches", "n", "best_iter", "best_count", "refine_status", "refine_steps")


def _pnp_record(ctx, c, begin_end):
    kw = dict(iters=c.iters, thr=PP.THR, seed=c.seed, refine=c.refine, want_matches=True, cross_check=c.cross)
    for a in ctx._pnp_out(True)[1]:
        a[:] = 0x5A                                        # nothing an earlier call left in the arrays passes for this one's output
    if begin_end:
        tk = ctx.pnp_pair_begin(0, 1, PP.RATIO, c.K4, **kw)
        for a in ctx._pnp_out(True)[1]:
            a[:] = 0x5A
        r = dict(ctx.pnp_pair_end(tk, want_matches=True))
    else:
        r = dict(ctx.pnp_pair(0, 1, PP.RATIO, c.K4, **kw))
    for k, a in zip(("mask", "q", "t"), ctx._pnp_arrays):
        r[k] = a[:c.nq].copy()                             # as the step wrote them for ALL nq query keypoints
    return r


def _pnp_body(roiname):
    from oracle import oracle as O
    ctx = _context(roiname)
    out = {}
    for c in [c for c in D.PNP_CASES if c.roiname == roiname]:
        def check():
            c.build()
            m = c.model(O)
            n = m["n"]
            ctx.set_Q(c.Q)
            ctx.plant_keypoints(0, c.xy_a, c.dq, c.xyz_a, c.rd_a)          # the sparse-planted twin: a's points are the lookup of every keypoint
            ctx.plant_keypoints(1, c.xy_b, c.dt, c.xyz_b, c.rd_b)
            twin = _pnp_record(ctx, c, False)
            assert twin["flags"] == 0
            ctx.plant_dense(0, c.disp_a, c.xy_a, c.dq)
            ctx.plant_dense(1, c.disp_b, c.xy_b, c.dt)
            want_flags = int((c.st_a[m["mq"]] == 2).any())
            for how, r in (("pnp_pair", _pnp_record(ctx, c, False)), ("pnp_pair_begin / _end", _pnp_record(ctx, c, True))):
                print("%s %s: (M, n, flags) = (%d, %d, %d) best %d @ %d; want (%d, %d, %d) best %d @ %d" % (
                    c.name, how, r["matches"], r["n"], r["flags"], r["best_count"], r["best_iter"], m["M"], n, want_flags, m["best_count"], m["best_iter"]), flush=True)
                assert (r["matches"], r["n"], r["flags"]) == (m["M"], n, want_flags), "%s: (M, n, flags) = (%d, %d, %d), want (%d, %d, %d)" % (
                    how, r["matches"], r["n"], r["flags"], m["M"], n, want_flags)
                assert np.array_equal(r["q"][:n], m["q"]) and np.array_equal(r["t"][:n], m["t"]), "%s: q / t differ from the status-0 filter of the matches" % how
                assert (r["q"][n:] == -1).all() and (r["t"][n:] == -1).all() and not r["mask"][n:].any(), "%s: the tails of mask / q / t" % how
                assert np.array_equal(r["mask"][:n], m["mask"]), "%s: mask differs from the oracle's" % how
                assert (r["best_iter"], r["best_count"]) == (m["best_iter"], m["best_count"]), "%s: best (%d, %d)" % (how, r["best_iter"], r["best_count"])
                d = float(np.abs(r["Rt"] - m["Rt"]).max())
                assert d <= BAR_RT, "%s: Rt differs from the oracle by %.3g" % (how, d)
                for k in PNP_SCALARS:
                    assert r[k] == twin[k], "%s: %s %s, the sparse-planted twin's %s" % (how, k, r[k], twin[k])
                for k in ("Rt", "Rt_refined", "mask", "q", "t"):
                    assert np.array_equal(r[k], twin[k]), "%s: %s is not bit-identical with the sparse-planted twin" % (how, k)
                if n >= 4:
                    # uv itself never leaves the device: ransac_pnp on the model's uv (= xy_b[t] + float32 origin) must give these very bits
                    ref = ctx.ransac_pnp(m["X"], m["uv"], c.K4, c.iters, PP.THR, c.seed)
                    assert np.array_equal(ref["Rt"], r["Rt"]) and np.array_equal(ref["mask"], r["mask"][:n]), "%s: not the pose of ransac_pnp on (X, xy_b[t] + origin)" % how
                    if c.roi is not None:                  # ... and NOT the pose without the origin: the add is really made
                        off = ctx.ransac_pnp(m["X"], c.xy_b[m["t"]], c.K4, c.iters, PP.THR, c.seed)
                        assert not np.array_equal(off["Rt"], r["Rt"])
                else:
                    assert not r["Rt"].any() and r["best_count"] == 0
            return dict(M=m["M"], n=n, flags=want_flags, best_count=m["best_count"], dRt=d)
        _run(out, c.name, check)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _refusals_body():
    from openvo_amd import _native
    from oracle import oracle as O
    roiname = "inner"
    ctx, roi = _context(roiname), D.ROIS[roiname]
    cw, ch = roi[2] - roi[0], roi[3] - roi[1]
    Q, disp = D.QS["plain"], D.FIELDS["hole_blocks"]()
    ctx.set_Q(Q)
    xy = D.positions("float", disp, Q, roi, 50)
    desc = np.random.default_rng(1).integers(0, 256, (50, 32), dtype=np.uint8)
    ctx.plant_dense(3, disp, xy, desc)
    probe = D.mixed_positions(disp, Q, roi, 200)
    before = ctx.points3d_at(3, probe)
    _same_lookup(*before, *O.points3d_at(disp, Q, _roi4(roi), probe), "before the refusals")
    other = D.FIELDS["smooth"]()                            # what a refused call would have planted: every probe would change
    good = np.float32([[1, 1], [2, 2]])
    d2 = np.zeros((2, 32), np.uint8)
    for bad in ([cw, 1], [1, ch], [-1, 1], [1, -0.5], [np.nan, 1], [1, np.inf], [3e9, 1]):
        with pytest.raises(_native.VoError) as e:
            ctx.plant_dense(3, other, np.float32([[1, 1], bad]), d2)
        assert e.value.code == VO_E_ARG, (bad, e.value)
    n = ctx.kp_cap + 1
    with pytest.raises(_native.VoError) as e:
        ctx.plant_dense(3, other, np.ones((n, 2), np.float32), np.zeros((n, 32), np.uint8))
    assert e.value.code == VO_E_CAP
    for shape in ((D.H, 15), (15, D.W), (D.H, D.W + 1), (D.H + 1, D.W)):
        with pytest.raises(_native.VoError) as e:
            ctx.plant_dense(3, np.full(shape, 100, np.int16), good, d2)
        assert e.value.code == VO_E_CAP, shape
    lib, vp = ctx._lib, ctypes.c_void_p
    pd, pxy, pde = vp(other.ctypes.data), vp(good.ctypes.data), vp(d2.ctypes.data)
    big = 2 ** 31 - 1
    assert lib.vo_test_plant_dense(None, 3, D.W, D.H, pd, 2, pxy, pde) == VO_E_ARG
    for args in ((3, D.W, D.H, None, 2, pxy, pde), (3, D.W, D.H, pd, 2, None, pde), (3, D.W, D.H, pd, 2, pxy, None), (3, D.W, D.H, None, 0, None, None),
                 (-1, D.W, D.H, pd, 2, pxy, pde), (_native.VO_NUM_SLOTS, D.W, D.H, pd, 2, pxy, pde), (big, D.W, D.H, pd, 2, pxy, pde),
                 (3, D.W, D.H, pd, -1, pxy, pde), (3, D.W, D.H, pd, -big - 1, pxy, pde)):
        assert lib.vo_test_plant_dense(ctx._h, *args) == VO_E_ARG, args
    for args in ((3, -5, D.H, pd, 2, pxy, pde), (3, D.W, 0, pd, 2, pxy, pde), (3, big, D.H, pd, 2, pxy, pde), (3, D.W, big, pd, 2, pxy, pde),
                 (3, -big - 1, -big - 1, pd, 2, pxy, pde), (3, D.W, D.H, pd, big, pxy, pde)):
        assert lib.vo_test_plant_dense(ctx._h, *args) == VO_E_CAP, args
    after = ctx.points3d_at(3, probe)
    assert np.array_equal(before[1], after[1]) and np.array_equal(_bits(before[0]), _bits(after[0])), "a refused call changed the slot"
    k = ctx.download_keypoints(3)
    assert np.array_equal(k["xy"], xy) and np.array_equal(k["desc"], desc)
    for name in ("size", "angle", "response", "octave"):
        assert len(k[name]) == 50 and not k[name].any(), name
    with pytest.raises(_native.VoError) as e:              # the keypoints of a dense slot carry no depth
        ctx.download_keypoint_depth(3)
    assert e.value.code == VO_E_STATE
    ctx.plant_dense(3, other, np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8))         # no keypoints at all: a valid dense slot
    _same_lookup(*ctx.points3d_at(3, probe), *O.points3d_at(other, Q, _roi4(roi), probe), "after planting again")
    ctx.close()
    ctx = _native.Context(0, D.W, D.H, 16, 1024)            # a ROI that leaves nothing of the image: refused, nothing planted
    ctx.set_Q(Q)
    ctx.set_roi(D.W - 6, 5, 200, 100)
    with pytest.raises(_native.VoError) as e:
        ctx.plant_dense(0, np.full((D.H, D.W - 6), 100, np.int16), np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8))
    assert e.value.code == VO_E_ARG
    with pytest.raises(_native.VoError) as e:
        ctx.points3d_at(0, good)
    assert e.value.code == VO_E_STATE
    ctx.close()
    print("PLANTED-RESULT {}")


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    """run tests.test_gpu_planted_dense.<body> once in a process of its own against the test-only library -> its result dict"""
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_planted_dense as t; t.%s" % body], cwd=ROOT,
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


LOOKUPS = [(r, f, q) for r in D.ROIS for f in D.FIELDS for q in D.QS]


@pytest.mark.parametrize("roiname,field,qname", LOOKUPS, ids=["-".join(c) for c in LOOKUPS])
def test_points3d_at(roiname, field, qname):
    res = _child("_lookup_body(%r)" % roiname)["%s-%s" % (field, qname)]
    assert res["ok"], res["err"]
    print("%s %s %s: %d lookups, status 0 / 1 / 2: %s" % (roiname, field, qname, res["n"], res["status"]))


@pytest.mark.parametrize("size", ["%dx%d" % s for s in DOWNLOAD_SIZES])
def test_downloads(size):
    res = _child("_download_body()")[size]
    assert res["ok"], res["err"]


CLOUD_IDS = ["nq%d-%s" % (c[0], f) for c in CLOUDS for f, _ in CLOUD_FIELDS] + ["dense_and_sparse"]


@pytest.mark.parametrize("name", CLOUD_IDS)
def test_point_clouds(name):
    res = _child("_clouds_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", [c.name for c in D.POSE_CASES])
def test_pose_pair(name):
    c = next(c for c in D.POSE_CASES if c.name == name)
    res = _child("_pose_body(%r)" % c.roiname)[name]
    assert res["ok"], res["err"]
    print("%s: (nq, M, n1, n2) = (%d, %d, %d, %d) flags %d, largest |T - numpy| = %.3g" % (name, res["nq"], res["M"], res["n1"], res["n2"], res["flags"], res["dT"]))


@pytest.mark.parametrize("name", [c.name for c in D.PNP_CASES])
def test_pnp_pair(name):
    c = next(c for c in D.PNP_CASES if c.name == name)
    res = _child("_pnp_body(%r)" % c.roiname)[name]
    assert res["ok"], res["err"]
    print("%s: (M, n, flags) = (%d, %d, %d) best_count %d, |Rt - oracle| = %.3g" % (name, res["M"], res["n"], res["flags"], res["best_count"], res["dRt"]))


def test_the_hook_refuses_and_leaves_the_slot_as_it_was():
    _child("_refusals_body()")
