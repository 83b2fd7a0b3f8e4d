"""The fused stereo PnP pair step (vo_pnp_pair / _begin / _end) on the GPU.

Held to (a) the composed path it replaces -- point_clouds -> host filter -> ransac_pnp, bit for bit; (b) the CPU oracle's
composition bf_knn2_hamming -> ratio_filter -> points3d_at -> ransac_pnp; (c) tests/pnp_refine_ref.py for the refinement; and,
through StereoOdometer, (d) the odometer that is forced onto the composed path and (e) the corridor's ground truth.
One native context serves the whole module (the T0 rig first, then the C1 rig on the same context)."""
import os
import sys

import numpy as np
import pytest

from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.synth import Corridor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_refine_ref as PR                # noqa: E402

pytestmark = pytest.mark.gpu

ITERS, THR, SEED, RATIO = 256, 1.5, 4321, 0.8
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4


def _camera(ctx, name):
    c = Corridor(name)
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)
    return c, cam


def _K4(cam):
    Q = cam.Q
    return [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]


def _frames(cam, odo, pairs):
    """each pair -> a frame resident in a slot: (handle that keeps the slot, KeyPointList)"""
    out = []
    for L, R in pairs:
        x3, disp, left = cam.compute_3d(L, R, preprocessed=True)
        kps, desc = odo.orb.detectAndCompute(left, odo.feature_mask(disp))
        assert len(kps) >= 30
        out.append((x3, kps))
    return out


def _composed(ctx, fa, fb, K4, ratio=RATIO, iters=ITERS, cross=False):
    """the path of the parent commit (StereoOdometer._pair_pnp) on two resident frames"""
    ka, kb = fa[1], fb[1]
    q, t, pa, _, sa, _ = ctx.point_clouds(ka.frame.slot, kb.frame.slot, ratio, cross)
    ok = (sa == 0) & np.isfinite(pa).all(axis=1)
    uv = kb.xy[t[ok]] + np.array([kb.frame.roi[0], kb.frame.roi[1]], np.float32)
    out = dict(M=len(q), flag=int((sa == 2).any()), q=q[ok], t=t[ok], X=pa[ok], uv=uv.astype(np.float32).reshape(-1, 2), r=None)
    if ok.sum() >= 4:
        out["r"] = ctx.ransac_pnp(pa[ok], uv, K4, iters, THR, SEED)
    return out


def _oracle_chain(oracle, cam, fa, fb, K4, ratio=RATIO, cross=False):
    ka, kb = fa[1], fb[1]
    da, db = cam._ctx.download_keypoints(ka.frame.slot), cam._ctx.download_keypoints(kb.frame.slot)
    idx, dist = oracle.bf_knn2_hamming(da["desc"], db["desc"])
    q, t = oracle.ratio_filter(idx, dist, ratio)
    if cross:
        back = oracle.bf_knn2_hamming(db["desc"], da["desc"])[0][:, 0]
        keep = back[t] == q
        q, t = q[keep], t[keep]
    disp16 = np.rint(ka.frame.full("disp") * 16).astype(np.int16)
    p, s = oracle.points3d_at(disp16, cam.Q, cam.valid_region_left, da["xy"][q])
    ok = (s == 0) & np.isfinite(p).all(axis=1)
    uv = db["xy"][t[ok]] + np.array([kb.frame.roi[0], kb.frame.roi[1]], np.float32)
    return dict(M=len(q), q=q[ok], t=t[ok], r=oracle.ransac_pnp(p[ok], uv, K4, ITERS, THR, SEED))


def _same_record(a, b):
    for k in ("matches", "n", "best_iter", "best_count", "flags", "refine_status", "refine_steps"):
        assert a[k] == b[k], k
    for k in ("Rt", "Rt_refined") + (("mask", "q", "t") if "mask" in a and "mask" in b else ()):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def rig(oracle):
    """One context; the T0 pairs are run and compared here (the context then belongs to the C1 camera), the C1 frames stay."""
    ctx = _native.Context(0, 640, 480, 64, 500)
    t0_rows = []
    c0, cam0 = _camera(ctx, "T0")
    odo0 = StereoOdometer(cam0, nfeatures=300, preprocessed_frames=True)
    fr0 = _frames(cam0, odo0, c0.pairs(0, 3))
    K40 = _K4(cam0)
    for a, b in zip(fr0[:-1], fr0[1:]):
        fused = ctx.pnp_pair(a[1].frame.slot, b[1].frame.slot, RATIO, K40, ITERS, THR, SEED, refine=5, want_matches=True)
        t0_rows.append((fused, _composed(ctx, a, b, K40), _oracle_chain(oracle, cam0, a, b, K40), K40))
    del fr0, odo0, cam0
    c, cam = _camera(ctx, "C1")
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True)
    pairs = c.pairs(0, 12)
    frames = _frames(cam, odo, pairs[:7])
    yield dict(ctx=ctx, c=c, cam=cam, odo=odo, pairs=pairs, frames=frames, K4=_K4(cam), t0_rows=t0_rows)
    del frames
    ctx.close()


@pytest.fixture(scope="module")
def c1_rows(rig, oracle):
    """fused (refine 5, with arrays), composed and oracle records of the C1 pairs: five plain, one with the cross-check"""
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    rows = []
    for k in range(6):
        cross = k == 5
        a, b = fr[k], fr[k + 1]
        fused = ctx.pnp_pair(a[1].frame.slot, b[1].frame.slot, RATIO, K4, ITERS, THR, SEED, refine=5, want_matches=True, cross_check=cross)
        rows.append((fused, _composed(ctx, a, b, K4, cross=cross), _oracle_chain(oracle, rig["cam"], a, b, K4, cross=cross), K4))
    return rows


def _check_rows(rows):
    for fused, comp, orc, _ in rows:
        r = comp["r"]
        assert fused["matches"] == comp["M"] and fused["n"] == len(comp["q"]) and fused["flags"] == comp["flag"] == 0
        assert np.array_equal(fused["q"], comp["q"]) and np.array_equal(fused["t"], comp["t"])
        assert fused["best_iter"] == r["best_iter"] and fused["best_count"] == r["best_count"]
        assert np.array_equal(fused["mask"], r["mask"])
        assert np.array_equal(fused["Rt"], r["Rt"])                           # the same arithmetic on the same inputs
        assert fused["n"] >= 30 and fused["best_count"] >= 10                   # (a real pair, not an empty one)
        o = orc["r"]
        assert fused["matches"] == orc["M"] and np.array_equal(fused["q"], orc["q"]) and np.array_equal(fused["t"], orc["t"])
        assert fused["best_iter"] == o["best_iter"] and fused["best_count"] == o["best_count"]
        assert np.array_equal(fused["mask"], o["mask"])
        assert np.abs(fused["Rt"] - np.asarray(o["Rt"]).reshape(3, 4)).max() <= 1e-10


def test_fused_equals_composed_and_oracle_bit_for_bit(rig, c1_rows):
    assert len(rig["t0_rows"]) + len(c1_rows) >= 7
    _check_rows(rig["t0_rows"])
    _check_rows(c1_rows)
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    plain = ctx.pnp_pair(fr[5][1].frame.slot, fr[6][1].frame.slot, RATIO, K4, ITERS, THR, SEED)
    assert c1_rows[5][0]["matches"] <= plain["matches"]                        # the cross-check only removes matches


def test_refinement_matches_the_restatement_per_pair(rig, c1_rows):
    """Rt12_refined within 1e-9 of the numpy restatement applied to the GPU's own winner, mask and arrays (the project's bar for
    a pose through reordered float64 sums); status and step count exact."""
    worst = 0.0
    for fused, comp, _, K4 in rig["t0_rows"] + c1_rows:
        ref, status, steps = PR.refine(fused["Rt"], comp["X"], comp["uv"], K4, fused["mask"], 5)
        err = float(np.abs(fused["Rt_refined"] - ref).max())
        worst = max(worst, err)
        print("pair: inliers %d, |refined - restatement| = %.3e, moved %.3e" % (fused["best_count"], err, np.abs(ref - fused["Rt"]).max()))
        assert (fused["refine_status"], fused["refine_steps"]) == (status, steps) == (0, 5)
        assert err <= 1e-9
        assert np.abs(ref - fused["Rt"]).max() > 1e-7                          # (the refinement does move the winner)
    print("worst %.3e" % worst)


def test_refine_zero_is_not_attempted_and_changes_nothing_else(rig, c1_rows):
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    r = ctx.pnp_pair(fr[0][1].frame.slot, fr[1][1].frame.slot, RATIO, K4, ITERS, THR, SEED, refine=0, want_matches=True)
    assert (r["refine_status"], r["refine_steps"]) == (1, 0)
    f5 = c1_rows[0][0]
    for k in ("matches", "n", "best_iter", "best_count"):
        assert r[k] == f5[k]
    assert np.array_equal(r["Rt"], f5["Rt"]) and np.array_equal(r["mask"], f5["mask"])   # the refinement changes nothing else


def test_begin_end_same_record_out_of_order_and_interleaved_with_pose_tickets(rig):
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    s = [f[1].frame.slot for f in fr]
    args = (RATIO, K4, ITERS, THR, SEED)
    sync = [ctx.pnp_pair(s[k], s[k + 1], *args, refine=3, want_matches=True) for k in range(3)]
    pose_sync = ctx.pose_pair(s[1], s[2], RATIO, 10, 0.1, 0.02)
    t0 = ctx.pnp_pair_begin(s[0], s[1], *args, refine=3, want_matches=True)
    tp = ctx.pose_pair_begin(s[1], s[2], RATIO, 10, 0.1, 0.02)
    t1 = ctx.pnp_pair_begin(s[1], s[2], *args, refine=3, want_matches=True)
    t2 = ctx.pnp_pair_begin(s[2], s[3], *args, refine=3, want_matches=False)
    assert len({t0, tp, t1, t2}) == 4
    # a ticket is ended by the _end of its kind: the wrong one is refused and leaves the ticket open
    with pytest.raises(_native.VoError) as e:
        ctx.pose_pair_end(t1)
    assert e.value.code == VO_E_STATE
    with pytest.raises(_native.VoError) as e:
        ctx.pnp_pair_end(tp)
    assert e.value.code == VO_E_STATE
    with pytest.raises(_native.VoError) as e:           # arrays asked of a step begun without them
        ctx.pnp_pair_end(t2, want_matches=True)
    assert e.value.code == VO_E_CAP
    _same_record(ctx.pnp_pair_end(t2), sync[2])
    _same_record(ctx.pnp_pair_end(t0, want_matches=True), sync[0])
    got = ctx.pose_pair_end(tp)
    assert all(np.array_equal(a, b) for a, b in zip(got, pose_sync) if a is not None)
    _same_record(ctx.pnp_pair_end(t1, want_matches=True), sync[1])
    with pytest.raises(_native.VoError) as e:           # ended twice
        ctx.pnp_pair_end(t1)
    assert e.value.code == VO_E_STATE


def test_every_alternate_open_is_a_state_error_and_pose_tickets_count(rig):
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    s = [f[1].frame.slot for f in fr]
    tickets = [("pnp", ctx.pnp_pair_begin(s[k % 6], s[k % 6 + 1], RATIO, K4, ITERS, THR, SEED)) for k in range(_native.VO_NUM_POSE_ASYNC - 2)]
    tickets += [("pose", ctx.pose_pair_begin(s[0], s[1], RATIO, 10, 0.1, 0.02)) for _ in range(2)]
    try:
        with pytest.raises(_native.VoError) as e:
            ctx.pnp_pair_begin(s[0], s[1], RATIO, K4, ITERS, THR, SEED)
        assert e.value.code == VO_E_STATE
        with pytest.raises(_native.VoError) as e:
            ctx.pose_pair_begin(s[0], s[1], RATIO, 10, 0.1, 0.02)
        assert e.value.code == VO_E_STATE
    finally:
        for kind, t in reversed(tickets):
            (ctx.pnp_pair_end if kind == "pnp" else ctx.pose_pair_end)(t)
    t = ctx.pnp_pair_begin(s[0], s[1], RATIO, K4, ITERS, THR, SEED)             # room again
    ctx.pnp_pair_end(t)


def test_refilling_a_slot_read_by_an_open_ticket_is_safe(rig):
    ctx, cam, odo, K4 = rig["ctx"], rig["cam"], rig["odo"], rig["K4"]
    a, b = _frames(cam, odo, rig["pairs"][7:9])
    sa, sb = a[1].frame.slot, b[1].frame.slot
    want = ctx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True)
    t = ctx.pnp_pair_begin(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True)
    L, R = rig["pairs"][11]
    ctx.upload_pair(sb, L, R, True)                     # the refill is ordered behind the ticket's work on the device
    ctx.sgbm_compute(sb)
    ctx.orb_slot_count(sb, *odo.orb.last_slot_args)
    _same_record(ctx.pnp_pair_end(t, want_matches=True), want)
    ctx.synchronize()


def test_edge_sizes(rig):
    ctx, fr, K4 = rig["ctx"], rig["frames"], rig["K4"]
    a, b = fr[2], fr[3]
    sa, sb = a[1].frame.slot, b[1].frame.slot
    # M = 0: no match passes a ratio of 0
    r = ctx.pnp_pair(sa, sb, 0.0, K4, ITERS, THR, SEED, refine=5, want_matches=True)
    assert (r["matches"], r["n"], r["best_iter"], r["best_count"], r["flags"]) == (0, 0, 0, 0, 0)
    assert not r["Rt"].any() and (r["refine_status"], r["refine_steps"]) == (1, 0) and len(r["mask"]) == 0
    # n = 3: the ratio that lets exactly three usable correspondences through (found on the composed path)
    idx, dist = ctx.bf_knn2(ctx.download_keypoints(sa)["desc"], ctx.download_keypoints(sb)["desc"])
    rat = np.sort(np.where(dist[:, 1] > 0, dist[:, 0] / np.maximum(dist[:, 1], 1).astype(np.float64), np.inf))
    ratio3 = None
    for m in range(3, 40):
        if rat[m - 1] < rat[m]:
            cand = 0.5 * (rat[m - 1] + rat[m])
            comp = _composed(ctx, a, b, K4, ratio=cand)
            if len(comp["q"]) == 3:
                ratio3 = cand
                break
    assert ratio3 is not None
    r = ctx.pnp_pair(sa, sb, ratio3, K4, ITERS, THR, SEED, refine=5, want_matches=True)
    assert r["matches"] == comp["M"] >= 3 and r["n"] == 3 and r["best_count"] == 0 and r["best_iter"] == 0
    assert not r["Rt"].any() and r["refine_status"] == 1
    assert np.array_equal(r["q"], comp["q"]) and np.array_equal(r["t"], comp["t"]) and not r["mask"].any()
    # iters = 1
    r = ctx.pnp_pair(sa, sb, RATIO, K4, 1, THR, SEED, refine=2, want_matches=True)
    comp = _composed(ctx, a, b, K4, iters=1)
    assert r["best_iter"] == 0 and r["best_count"] == comp["r"]["best_count"]
    assert np.array_equal(r["Rt"], comp["r"]["Rt"]) and np.array_equal(r["mask"], comp["r"]["mask"])
    assert (r["refine_status"] != 1) == (r["best_count"] >= 6)                  # attempted exactly from six inliers on


def test_state_and_hostile_arguments_give_a_status(rig):
    ctx, cam, fr, K4 = rig["ctx"], rig["cam"], rig["frames"], rig["K4"]
    sa, sb = fr[0][1].frame.slot, fr[1][1].frame.slot
    L, R = rig["pairs"][9]
    x3, disp, left = cam.compute_3d(L, R, preprocessed=True)                    # a pair with disparity and no keypoints
    bare = x3.frame.slot

    def code(fn, *a, **kw):
        with pytest.raises(_native.VoError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(ctx.pnp_pair, sa, bare, RATIO, K4, ITERS, THR, SEED) == VO_E_STATE
    assert code(ctx.pnp_pair, bare, sb, RATIO, K4, ITERS, THR, SEED) == VO_E_STATE
    assert code(ctx.pnp_pair_begin, sa, bare, RATIO, K4, ITERS, THR, SEED) == VO_E_STATE
    for a, b in ((-1, sb), (sa, -1), (_native.VO_NUM_SLOTS, sb), (sa, 2 ** 31 - 1), (-2 ** 31, sb)):
        assert code(ctx.pnp_pair, a, b, RATIO, K4, ITERS, THR, SEED) == VO_E_ARG
        assert code(ctx.pnp_pair_begin, a, b, RATIO, K4, ITERS, THR, SEED) == VO_E_ARG
    for iters in (0, -1, 2 ** 22 + 1, 2 ** 31 - 1, -2 ** 31):
        assert code(ctx.pnp_pair, sa, sb, RATIO, K4, iters, THR, SEED) == VO_E_ARG
        assert code(ctx.pnp_pair_begin, sa, sb, RATIO, K4, iters, THR, SEED) == VO_E_ARG
    for refine in (-1, 21, 2 ** 31 - 1, -2 ** 31):
        assert code(ctx.pnp_pair, sa, sb, RATIO, K4, ITERS, THR, SEED, refine=refine) == VO_E_ARG
        assert code(ctx.pnp_pair_begin, sa, sb, RATIO, K4, ITERS, THR, SEED, refine=refine) == VO_E_ARG
    assert code(ctx.pnp_pair, sa, sb, RATIO, K4, ITERS, 0.0, SEED) == VO_E_ARG
    assert code(ctx.pnp_pair, sa, sb, RATIO, K4, ITERS, float("nan"), SEED) == VO_E_ARG
    assert code(ctx.pnp_pair, sa, sb, RATIO, [0.0, 400.0, 320.0, 240.0], ITERS, THR, SEED) == VO_E_ARG
    for ticket in (-1, _native.VO_NUM_POSE_ASYNC, 2 ** 31 - 1, -2 ** 31):
        assert code(ctx.pnp_pair_end, ticket) == VO_E_ARG
    assert code(ctx.pnp_pair_end, 0) == VO_E_STATE                              # nothing open
    # raw entry: a NULL pointer, unknown match flags, outputs that are too short
    lib, h = ctx._lib, ctx._h
    K = np.asarray(K4, np.float64)
    c4, fl, Rt, r2 = np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(12), np.zeros(2, np.int32)
    p = _native._p
    small = np.zeros(4, np.uint8)
    assert lib.vo_pnp_pair(h, sa, sb, RATIO, 0, None, ITERS, THR, SEED, 0, p(c4), p(fl), p(Rt), None, p(r2), None, None, None, 0) == VO_E_ARG
    assert lib.vo_pnp_pair(h, sa, sb, RATIO, 0, p(K), ITERS, THR, SEED, 0, None, p(fl), p(Rt), None, p(r2), None, None, None, 0) == VO_E_ARG
    assert lib.vo_pnp_pair(h, sa, sb, RATIO, 2, p(K), ITERS, THR, SEED, 0, p(c4), p(fl), p(Rt), None, p(r2), None, None, None, 0) == VO_E_ARG
    assert lib.vo_pnp_pair(h, sa, sb, RATIO, 0, p(K), ITERS, THR, SEED, 0, p(c4), p(fl), p(Rt), None, p(r2), p(small), None, None, 4) == VO_E_CAP
    assert lib.vo_pnp_pair_begin(h, sa, sb, RATIO, 0, p(K), ITERS, THR, SEED, 0, 0, None) == VO_E_ARG
    # and the context still works
    r = ctx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED)
    assert r["best_count"] >= 10


@pytest.fixture(scope="module")
def composed_chain(rig):
    """the odometer forced onto the composed path, C1, 12 pairs: the reference of the two fused chains"""
    odo = StereoOdometer(rig["cam"], preprocessed_frames=True, pose_method="pnp")
    odo._pnp_fused = False
    out = []
    for L, R in rig["pairs"]:
        out.append((odo.update(L, R), odo.skip_cause, odo.c_T_w.copy()))
    return out


def test_odometer_update_equals_the_composed_path(rig, composed_chain):
    odo = StereoOdometer(rig["cam"], preprocessed_frames=True, pose_method="pnp")
    for k, (L, R) in enumerate(rig["pairs"]):
        got = (odo.update(L, R), odo.skip_cause, odo.c_T_w.copy())
        want = composed_chain[k]
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), k
    assert all(w[0] for w in composed_chain)


def test_odometer_run_with_lookahead_equals_the_composed_path(rig, composed_chain):
    """run() under the default look-ahead: PnP steps are begun ahead on the pose alternates and collected by their key"""
    odo = StereoOdometer(rig["cam"], preprocessed_frames=True, pose_method="pnp")
    got = [(ok, odo.skip_cause, odo.c_T_w.copy()) for ok in odo.run(iter(rig["pairs"]))]
    assert len(got) == len(composed_chain)
    for k, (g, w) in enumerate(zip(got, composed_chain)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]), k
    assert all(k[2][0] == "pnp" for k in odo._specs)
    odo.reset_lookahead()
    assert not odo._specs


def test_a_step_begun_ahead_is_collected_by_the_next_update(rig, composed_chain):
    """What run() does when the next pair is already on the device, made deterministic: the pair is submitted and waited for,
    _start_next_pose begins its PnP step on a pose alternate, update() collects that ticket instead of computing."""
    cam, ctx, pairs = rig["cam"], rig["ctx"], rig["pairs"]
    odo = StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp")
    ended = []
    real_end = ctx.pnp_pair_end
    ctx.pnp_pair_end = lambda t, **kw: ended.append(t) or real_end(t, **kw)
    try:
        assert odo.update(*pairs[0])
        for k in range(1, 5):
            sp = cam.submit(pairs[k][0], pairs[k][1], preprocessed=True)
            ctx.synchronize()
            odo._next_hint = (sp,)
            odo._start_next_pose()
            odo._next_hint = ()
            assert len(odo._specs) == 1 and next(iter(odo._specs))[2][0] == "pnp"
            assert odo.update(sp, None) == composed_chain[k][0]
            assert len(ended) == k and not odo._specs
            assert np.array_equal(odo.c_T_w, composed_chain[k][2]), k
    finally:
        del ctx.pnp_pair_end
        odo.reset_lookahead()


def test_odometer_with_cross_check_equals_the_composed_path(rig):
    """cross_check=True reaches the fused step (and the steps begun ahead) as the cross-check, not as anything else: update()
    and run() equal the composed path, which differs from the chain without the cross-check."""
    kw = dict(preprocessed_frames=True, pose_method="pnp", cross_check=True)
    ref = StereoOdometer(rig["cam"], **kw)
    ref._pnp_fused = False
    want = [(ref.update(L, R), ref.skip_cause, ref.c_T_w.copy()) for L, R in rig["pairs"]]
    odo = StereoOdometer(rig["cam"], **kw)
    for k, (L, R) in enumerate(rig["pairs"]):
        got = (odo.update(L, R), odo.skip_cause, odo.c_T_w.copy())
        assert got[0] == want[k][0] and got[1] == want[k][1] and np.array_equal(got[2], want[k][2]), k
    odo = StereoOdometer(rig["cam"], **kw)
    got = [(ok, odo.skip_cause, odo.c_T_w.copy()) for ok in odo.run(iter(rig["pairs"]))]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]), k
    odo.reset_lookahead()
    # begun ahead, deterministically (see test_a_step_begun_ahead_is_collected_by_the_next_update)
    cam, ctx, pairs = rig["cam"], rig["ctx"], rig["pairs"]
    odo = StereoOdometer(cam, **kw)
    assert odo.update(*pairs[0])
    for k in range(1, 4):
        sp = cam.submit(pairs[k][0], pairs[k][1], preprocessed=True)
        ctx.synchronize()
        odo._next_hint = (sp,)
        odo._start_next_pose()
        odo._next_hint = ()
        assert len(odo._specs) == 1
        assert odo.update(sp, None) == want[k][0] and np.array_equal(odo.c_T_w, want[k][2]), k
    odo.reset_lookahead()
    plain = StereoOdometer(cam, preprocessed_frames=True, pose_method="pnp")
    for L, R in pairs:
        plain.update(L, R)
    assert not np.array_equal(plain.c_T_w, want[-1][2])                        # (the cross-check does change this chain)


def _refused_index_body():
    """Body of test_a_match_index_outside_the_train_set_refuses_the_pair: own process, test-only build of the library.
    VO_FAULT_PNP_RANGE=n makes the n-th PnP step of a context hold its match indices to a train set of one descriptor: the
    path of a corrupted kNN result, reached without corrupting anything."""
    os.environ["VO_FAULT_PNP_RANGE"] = "2"
    ctx = _native.Context(0, 640, 480, 64, 500)
    os.environ["VO_FAULT_PNP_RANGE"] = "3"
    ctx2 = _native.Context(0, 640, 480, 64, 500)
    del os.environ["VO_FAULT_PNP_RANGE"]
    for cx, sync in ((ctx, True), (ctx2, False)):
        c, cam = _camera(cx, "C1")
        odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True)
        fr = _frames(cam, odo, c.pairs(0, 2))
        sa, sb, K4 = fr[0][1].frame.slot, fr[1][1].frame.slot, _K4(cam)
        good = cx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True)          # step 1
        assert good["flags"] == 0 and good["best_count"] >= 10
        if sync:
            with pytest.raises(_native.VoError) as e:                                                # step 2: refused
                cx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True)
        else:
            _same_record(cx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True), good)   # step 2
            t = cx.pnp_pair_begin(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True)  # step 3: refused at _end
            with pytest.raises(_native.VoError) as e:
                cx.pnp_pair_end(t, want_matches=True)
        assert e.value.code == VO_E_STATE and "outside the train set" in str(e.value)
        _same_record(cx.pnp_pair(sa, sb, RATIO, K4, ITERS, THR, SEED, refine=3, want_matches=True), good)      # and the next one is exact
        del fr
        cx.close()
    print("refused-index body ok")


def test_a_match_index_outside_the_train_set_refuses_the_pair():
    """Flag bit 1: a refused pair (VO_E_STATE), never a wrong pose -- from the synchronous call and from _end, and the step
    after it is exact again."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "openvo_amd", "libvo355_hooks.so")
    assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_pnp_pair as t; t._refused_index_body()"], cwd=root,
                       env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused-index body ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refinement_improves_the_end_point_for_every_seed(rig):
    """C1, 12 pairs: the end-point error against the corridor's ground truth is smaller with pnp_refine=3 than with 0 for each
    of the eight RANSAC seeds (CPU oracle chain with this camera's valid region: 8 of 8, ratios 0.28 .. 0.88)."""
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(11)
    rows = []
    for seed in (4321, 1, 2, 3, 4, 5, 6, 7):
        e = []
        for refine in (0, 3):
            odo = StereoOdometer(rig["cam"], preprocessed_frames=True, pose_method="pnp", pnp_seed=seed, pnp_refine=refine)
            for L, R in rig["pairs"]:
                assert odo.update(L, R)
            e.append(float(np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3])))
        rows.append((seed, e[0], e[1]))
        print("seed %d: end-point error %.5f m -> %.5f m (ratio %.3f)" % (seed, e[0], e[1], e[1] / e[0]))
    for seed, e0, e3 in rows:
        assert e3 < e0, (seed, e0, e3)
