"""The landmark map on the GPU (csrc/map.hip: k_map_view, k_map_update) against the numpy restatement (tests/map_ref.py), bit for bit,
with landmarks and keypoints PLANTED through the test-only library (vo_test_plant_map / vo_test_plant_keypoints) so that the counts
hit the boundaries of the ballot compaction -- one workgroup of 1024 threads = 16 waves, trips of 1024 entries:

    view      visible counts 0, 1, 63, 64, 65, 1023, 1024, 1025 and capacity (= kp_cap = 3024): under one wave, one wave, a wave and
              one, under one trip, one trip, a trip and one, three trips that keep everything.  The pose has a rotation, the ROI
              origin is not zero; around every visibility boundary (u = 0, u = crop_w - 1, v = 0, v = crop_h - 1, z = z_min) a run
              of neighbouring float32 positions is planted, on both sides, with NaN, +-inf and z < 0 landmarks in between; one
              more case has landmarks EXACTLY on the four edges and one float32 outside them.  Then pnp_pair(view, new frame,
              want_matches=True): matches, n, mask, winner and count equal numpy matches + oracle.ransac_pnp on the restated view,
              Rt to 1e-10 (the bar of tests/test_gpu_planted_pnp.py).
    update    n in {0, 1, 64, 65, 1024, 1025}; survivors + insertions below, at, one above and 70 above capacity; all landmarks
              culled at once; every keypoint claimed (no insertion); two landmarks claiming one keypoint; max_obs reached;
              non-finite observations and non-finite unclaimed keypoints; three updates in a row (both sets of arrays are read
              and written), then a view of the result.  Every array, the order and all six counts.
    refusals  a status each and the map unchanged afterwards.
    odometer  StereoOdometer(track="map") on C1 frames 0-7, plain and with cross-check + match window, against the CPU chain
              MapRefOdometer (decisions, track_source, counts exactly; c_T_w to 1e-9, the bar of tests/test_gpu_sparse_stereo.py),
              run() against update(), a track="pair" odometer on the same camera before and after against the pairwise CPU
              chain; loop_check and pnp_refine compose.

The planted cases run in one child process per group, VO355_LIB pointing at the test-only library (as tests/test_gpu_planted_pnp.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_ref as M                        # noqa: E402
import planted as P                        # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX_KP = 704, 512, 1000
KP_CAP = 2 * MAX_KP + 1024                 # 3024
ROI = (24, 16, 680, 500)                   # origin (24, 16), crop 656 x 484
ORG, CROP = (24, 16), (656, 484)
K4 = (500.0, 500.0, 352.0, 256.0)
Z_MIN = 0.1
RATIO, ITERS, THR, SEED = 0.8, 256, 1.5, 4321
BAR_RT = 1e-10
VIEW_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, KP_CAP)
VIEW_SLOT, NEW_SLOT, REF_SLOT = 3, 5, 5    # (the new frame is the frame the view is placed for)
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4


def _rot(axis, angle):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose_cw():
    """world -> camera: a rotation about a skew axis and a translation"""
    return np.hstack([_rot((0.2, 1.0, 0.1), 0.12), np.array([[0.3], [-0.1], [0.4]])])


def _inv34(Rt):
    T = np.vstack([Rt, [0, 0, 0, 1]])
    return np.linalg.inv(T)[:3]


def _to_world(Xc):
    Rt = pose_cw()
    return ((np.asarray(Xc, np.float64) - Rt[:, 3]) @ Rt[:, :3]).astype(np.float32)


def _cam_point(u, v, z):
    """camera coordinates of crop pixel (u, v) at depth z"""
    return np.stack([(u + ORG[0] - K4[2]) / K4[0] * z, (v + ORG[1] - K4[3]) / K4[1] * z, z * np.ones_like(u)], -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _descs(n, rng):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the view scenes
def view_candidates(rng):
    """-> (xyz (n, 3) float32 world, kind): interior points, runs of neighbouring float32 positions across each visibility
    boundary, and points no view may show"""
    pts = []
    n_in = KP_CAP
    u, v, z = rng.uniform(2, CROP[0] - 3, n_in), rng.uniform(2, CROP[1] - 3, n_in), rng.uniform(1.0, 12.0, n_in)
    pts.append(_to_world(_cam_point(u, v, z)))
    for (bu, bv, bz), axis in ((((CROP[0] - 1.0), 200.0, 4.0), 0), ((0.0, 300.0, 3.0), 0), ((100.0, CROP[1] - 1.0, 5.0), 1), ((500.0, 0.0, 2.5), 1),
                               ((300.0, 250.0, Z_MIN), 2)):
        base = _to_world(_cam_point(np.array([bu]), np.array([bv]), bz))[0]
        run = np.tile(base, (161, 1))
        x = base[axis]
        lo = x
        for _ in range(80):
            lo = np.nextafter(lo, np.float32(-np.inf))
        vals = [lo]
        for _ in range(160):
            vals.append(np.nextafter(vals[-1], np.float32(np.inf)))
        run[:, axis] = np.array(vals, np.float32)
        pts.append(run)
    bad = [[np.nan, 0, 3], [0, np.nan, 3], [0, 0, np.nan], [np.inf, 0, 3], [-np.inf, 0, 3], [0, np.inf, 3], [0, 0, np.inf], [0, 0, -np.inf],
           [np.nan, np.nan, np.nan]]
    pts.append(np.array(bad, np.float32))
    behind = _cam_point(rng.uniform(0, CROP[0], 40), rng.uniform(0, CROP[1], 40), -rng.uniform(0.5, 9, 40))
    outside = np.concatenate([_cam_point(rng.uniform(-400, -1, 30), rng.uniform(0, CROP[1], 30), 4.0), _cam_point(rng.uniform(CROP[0] + 1, 1200, 30), rng.uniform(0, CROP[1], 30), 4.0),
                              _cam_point(rng.uniform(0, CROP[0], 30), rng.uniform(-300, -1, 30), 4.0), _cam_point(rng.uniform(0, CROP[0], 30), rng.uniform(CROP[1] + 1, 900, 30), 4.0)])
    pts.append(_to_world(np.concatenate([behind, outside])))
    kind = np.concatenate([np.full(len(p), k) for k, p in enumerate(pts)])
    return np.concatenate(pts).astype(np.float32), kind


def view_scene(V):
    """a planted map of which EXACTLY V landmarks are visible under pose_cw() (the restatement decides), shuffled"""
    rng = np.random.default_rng([7, V])
    xyz, kind = view_candidates(rng)
    probe = M.MapRef(len(xyz))
    n = len(xyz)
    probe.plant(xyz, np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n), np.ones(n), np.zeros(n))
    vis = np.zeros(n, bool)
    vis[probe.view(pose_cw(), K4, Z_MIN, ORG, CROP)["src"]] = True
    edge = (kind >= 1) & (kind <= 5)
    # visible: the boundary runs first (as many as fit), then interior points; invisible: everything that is not
    vis_pick = np.concatenate([rng.permutation(np.flatnonzero(vis & edge)), np.flatnonzero(vis & ~edge)])[:V]
    assert len(vis_pick) == V
    inv = rng.permutation(np.flatnonzero(~vis))
    inv_pick = inv[:min(len(inv), KP_CAP - V)]
    pick = rng.permutation(np.concatenate([vis_pick, inv_pick]))
    n = len(pick)
    return dict(xyz=xyz[pick], desc=_descs(n, rng), rdesc=_descs(n, rng), octave=rng.integers(0, 8, n).astype(np.int32),
                obs=rng.integers(1, 12, n).astype(np.int32), last=rng.integers(0, 6, n).astype(np.int32), capacity=KP_CAP)


def edge_scene():
    """identity pose, fx = fy = 1, cx = cy = 0, z = 1: the pixel IS float32(x) - origin, so landmarks lie exactly ON the four edges
    of the crop and one float32 outside them"""
    ox, oy = np.float32(ORG[0]), np.float32(ORG[1])
    e, f = np.float32(CROP[0] - 1) + ox, np.float32(CROP[1] - 1) + oy
    up, dn = (lambda x: np.nextafter(np.float32(x), np.float32(np.inf))), (lambda x: np.nextafter(np.float32(x), np.float32(-np.inf)))
    pts = [[e, 100, 1], [up(e), 100, 1], [ox, 100, 1], [dn(ox), 100, 1], [100, f, 1], [100, up(f), 1], [100, oy, 1], [100, dn(oy), 1],
           [e, f, 1], [ox, oy, 1], [up(e), up(f), 1], [100, 100, np.float32(Z_MIN)], [100, 100, dn(np.float32(Z_MIN))]]
    # (at z = z_min the pixel is 10 x: far outside -- the z boundary at a visible pixel is the business of the run in view_candidates)
    rng = np.random.default_rng(11)
    n = len(pts)
    return dict(xyz=np.array(pts, np.float32), desc=_descs(n, rng), rdesc=_descs(n, rng), octave=np.arange(n, dtype=np.int32) % 8,
                obs=np.ones(n, np.int32), last=np.zeros(n, np.int32), capacity=64)


def new_frame(view, rng, M_want=400, extra=7, noise=0.3):
    """the frame a view is matched against: M of the view's keypoints seen again (descriptors with up to two bits flipped) from a
    camera moved by planted._motion(), seven in ten at their projection (+ noise), the others anywhere; its own 3-D points too"""
    V = len(view["xy"])
    Mw = min(V, M_want)
    nt = max(Mw + extra, 2)
    desc = _descs(nt, rng)
    q = np.sort(rng.choice(V, Mw, replace=False)) if Mw else np.zeros(0, np.int64)
    t = rng.permutation(nt)[:Mw]
    R, tv = P._motion()
    xy = np.stack([rng.uniform(0, CROP[0], nt), rng.uniform(0, CROP[1], nt)], 1)
    xyz = P._cloud(nt, rng)
    for k in range(Mw):
        desc[t[k]] = view["desc"][q[k]]
        for bit in rng.choice(256, int(rng.integers(0, 3)), replace=False):
            desc[t[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
        Y = R @ view["xyz"][q[k]].astype(np.float64) + tv
        xyz[t[k]] = Y + rng.normal(0, 1e-3, 3)
        if rng.random() < 0.7:
            xy[t[k]] = [K4[0] * Y[0] / Y[2] + K4[2] - ORG[0] + noise * rng.normal(), K4[1] * Y[1] / Y[2] + K4[3] - ORG[1] + noise * rng.normal()]
    return dict(xy=xy.astype(np.float32), desc=desc, xyz=xyz.astype(np.float32), rdesc=_descs(nt, rng), octave=np.zeros(nt, np.int32))


def pnp_model(O, view, frame):
    """numpy matches + the finite filter + oracle.ransac_pnp on the restated view"""
    q, t = P.matches(view["desc"], frame["desc"], RATIO)
    X = view["xyz"][q]
    ok = np.isfinite(X).all(1)
    q, t, X = q[ok], t[ok], np.ascontiguousarray(X[ok])
    uv = np.ascontiguousarray(frame["xy"][t] + np.float32(ORG)).astype(np.float32).reshape(-1, 2)
    m = dict(M=len(ok), n=len(q), q=q, t=t)
    if len(q) >= 4:
        r = O.ransac_pnp(X, uv, K4, ITERS, THR, SEED)
        m.update(best_iter=r["best_iter"], best_count=r["best_count"], Rt=np.array(r["Rt"]).reshape(3, 4), mask=r["mask"].copy())
    else:
        m.update(best_iter=0, best_count=0, Rt=np.zeros((3, 4)), mask=np.zeros(len(q), np.uint8))
    return m


# ---------------------------------------------------------------------------------------------- in the child process
def _context():
    from openvo_amd import _native
    ctx = _native.Context(0, W, H, 16, MAX_KP)
    assert ctx.kp_cap == KP_CAP
    Q = np.eye(4)
    Q[3, 3] = 0.0; Q[2, 3] = 50.0; Q[3, 2] = 10.0
    ctx.set_Q(Q)
    ctx.set_roi(*ROI)
    blank = np.zeros((H, W), np.uint8)
    ctx.upload_pair(REF_SLOT, blank, blank, True)        # (the frame slot holds an image: its crop places the views)
    return ctx


def _plant_both(ctx, h, ref, s):
    ctx.plant_map(h, s["xyz"], s["desc"], s["rdesc"], s["octave"], s["obs"], s["last"])
    ref.plant(s["xyz"], s["desc"], s["rdesc"], s["octave"], s["obs"], s["last"])


def _same_view(ctx, got_c2, want, slot=VIEW_SLOT):
    assert tuple(got_c2) == tuple(want["counts2"]), "counts2 %s, want %s" % (tuple(got_c2), tuple(want["counts2"]))
    k = ctx.download_keypoints(slot)
    xyz, disp = ctx.download_keypoint_depth(slot)
    rdesc = ctx.download_keypoint_rdesc(slot)
    n = len(want["xy"])
    assert len(k["xy"]) == len(xyz) == len(rdesc) == n, "the slot holds %d keypoints, want %d" % (len(k["xy"]), n)
    assert np.array_equal(_bits(k["xy"]), _bits(want["xy"])), "kp_xy differs in %d places" % int((_bits(k["xy"]) != _bits(want["xy"])).any(1).sum())
    assert np.array_equal(_bits(xyz), _bits(want["xyz"])), "kp_xyz differs in %d places" % int((_bits(xyz) != _bits(want["xyz"])).any(1).sum())
    assert np.array_equal(k["desc"], want["desc"]) and np.array_equal(rdesc, want["rdesc"]), "descriptors differ"
    assert np.array_equal(k["octave"], want["octave"]), "octaves differ"
    assert not k["size"].any() and not k["angle"].any() and not k["response"].any(), "size / angle / response are not 0"
    assert np.isnan(disp).all(), "the disparities are not NaN"


def _same_map(ctx, h, ref):
    got, want = ctx.map_download(h), ref.download()
    assert len(got["xyz"]) == len(want["xyz"]), "the map holds %d landmarks, want %d" % (len(got["xyz"]), len(want["xyz"]))
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"])), "xyz differs in %d places" % int((_bits(got["xyz"]) != _bits(want["xyz"])).any(1).sum())
    for k in ("desc", "octave", "obs", "last"):
        assert np.array_equal(got[k], want[k]), "%s differs" % k


def _guard(out, name, fn):
    try:
        out[name] = dict(ok=True, **(fn() or {}))
    except AssertionError as e:                        # (anything else -- a native error status, a fault -- ends the child)
        out[name] = dict(ok=False, err=str(e)[:1500])
        print("%s: FAILED %s" % (name, out[name]["err"]), flush=True)


def _view_case(ctx, O, name, scene, pose, k4, pnp=True):
    h = ctx.map_create(scene["capacity"])
    try:
        ref = M.MapRef(scene["capacity"], KP_CAP)
        _plant_both(ctx, h, ref, scene)
        want = ref.view(pose, k4, Z_MIN, ORG, CROP)
        c2 = ctx.map_view(h, pose, k4, Z_MIN, REF_SLOT if not pnp else NEW_SLOT, VIEW_SLOT)
        _same_view(ctx, c2, want)
        fig = dict(size=int(c2[0]), visible=int(c2[1]))
        if pnp:
            rng = np.random.default_rng([13, len(want["xy"])])
            f = new_frame(want, rng)
            ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
            m = pnp_model(O, want, f)
            r = ctx.pnp_pair(VIEW_SLOT, NEW_SLOT, RATIO, K4, ITERS, THR, SEED, 0, True)
            assert (r["matches"], r["n"], r["flags"]) == (m["M"], m["n"], 0), "(M, n, flags) = (%d, %d, %d), want (%d, %d, 0)" % (
                r["matches"], r["n"], r["flags"], m["M"], m["n"])
            assert np.array_equal(r["q"], m["q"]) and np.array_equal(r["t"], m["t"]), "q / t differ from the numpy matches"
            assert np.array_equal(r["mask"], m["mask"]), "mask differs from the oracle's"
            assert (r["best_iter"], r["best_count"]) == (m["best_iter"], m["best_count"]), "best (%d, %d), want (%d, %d)" % (
                r["best_iter"], r["best_count"], m["best_iter"], m["best_count"])
            d = float(np.abs(r["Rt"] - m["Rt"]).max())
            assert d <= BAR_RT, "Rt differs from the oracle by %.3g" % d
            fig.update(M=m["M"], n=m["n"], best_count=m["best_count"], dRt=d)
        print("%s: %s" % (name, fig), flush=True)
        return fig
    finally:
        ctx.map_destroy(h)


def _view_body():
    from oracle import oracle as O
    O.build_oracle()
    ctx = _context()
    out = {}
    for V in VIEW_COUNTS:
        _guard(out, "visible%d" % V, lambda: _view_case(ctx, O, "visible%d" % V, view_scene(V), pose_cw(), K4))
    _guard(out, "exact_edges", lambda: _view_case(ctx, O, "exact_edges", edge_scene(), np.eye(4)[:3], (1.0, 1.0, 0.0, 0.0), pnp=False))
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---- update
class UpdateCase:
    """n0 planted landmarks, nk keypoints in the frame, n matches; delta: capacity - (survivors + wanted insertions) of the FIRST
    update; cull: how many landmarks are too old before it ("all": every one, and none is observed)"""

    def __init__(self, name, n0, nk, n, delta, cull=40, max_obs=8, claim_all=False):
        self.name, self.n0, self.nk, self.n, self.delta, self.cull, self.max_obs, self.claim_all = name, n0, nk, n, delta, cull, max_obs, claim_all


UPDATE_CASES = [
    UpdateCase("n0_first_frame_below_capacity", 0, 700, 0, +5),
    UpdateCase("n1_at_capacity", 300, 260, 1, 0),
    UpdateCase("n64_one_above_capacity", 300, 260, 64, -1),
    UpdateCase("n65_70_above_capacity", 300, 330, 65, -70),
    UpdateCase("n1024_below_capacity", 1500, 1200, 1024, +5),
    UpdateCase("n1025_70_above_capacity", 1500, 1300, 1025, -70, max_obs=2),
    UpdateCase("all_culled_at_once", 1100, 300, 0, +5, cull="all"),
    UpdateCase("every_keypoint_claimed", 600, 200, 200, 0, cull=0, claim_all=True),
]
MAX_AGE = 5


def _map_scene(n0, rng, serial, cull):
    Xc = _cam_point(rng.uniform(1, CROP[0] - 2, n0), rng.uniform(1, CROP[1] - 2, n0), rng.uniform(1.0, 12.0, n0)).reshape(n0, 3)
    last = rng.integers(serial - MAX_AGE, serial, n0)
    if cull == "all":
        last[:] = serial - MAX_AGE - 1 - rng.integers(0, 3, n0)
    elif n0:
        old = rng.choice(n0, min(cull, n0), replace=False)
        last[old] = serial - MAX_AGE - 1
        last[old[:len(old) // 4]] = serial - MAX_AGE          # (exactly max_age old: kept)
    return dict(xyz=_to_world(Xc), desc=_descs(n0, rng), rdesc=_descs(n0, rng), octave=rng.integers(0, 8, n0).astype(np.int32),
                obs=rng.integers(1, 12, n0).astype(np.int32), last=last.astype(np.int32))


def _frame_for(rng, nk):
    """nk keypoints with their 3-D points in the new camera's frame; about one in twelve has no finite point"""
    xyz = P._cloud(nk, rng).astype(np.float32)
    bad = np.flatnonzero(rng.random(nk) < 1 / 12)
    for k, i in enumerate(bad):
        xyz[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    return dict(xy=np.stack([rng.uniform(0, CROP[0], nk), rng.uniform(0, CROP[1], nk)], 1).astype(np.float32), desc=_descs(nk, rng), xyz=xyz,
                rdesc=_descs(nk, rng), octave=np.zeros(nk, np.int32))


def _matches_for(rng, n, n_view, nk, claim_all=False):
    """n distinct view keypoints against keypoints of the frame, four in five inliers; the first two name ONE keypoint"""
    n = min(n, n_view)
    q = rng.choice(n_view, n, replace=False).astype(np.int32)
    if claim_all:
        t, mask = rng.permutation(nk)[:n].astype(np.int32), np.ones(n, np.uint8)
    else:
        t, mask = rng.integers(0, nk, n).astype(np.int32), (rng.random(n) < 0.8).astype(np.uint8)
        if n >= 2:
            t[1] = t[0]
            mask[:2] = 1
    return q, t, mask


def _update_case(ctx, c):
    rng = np.random.default_rng([17, c.n0, c.nk, c.n])
    serial = 20
    scene = _map_scene(c.n0, rng, serial, c.cull)
    pose = pose_cw()
    wc = _inv34(pose)
    frames = [_frame_for(rng, c.nk), _frame_for(rng, max(40, c.nk // 3)), _frame_for(rng, 50)]
    if c.claim_all:
        frames[0]["xyz"] = P._cloud(c.nk, rng).astype(np.float32)         # (every keypoint claimed AND finite: nothing is left to insert)
    # the first update under an unbounded capacity tells what it keeps and wants: the capacity of the case follows from that
    probe = M.MapRef(KP_CAP + 4000, KP_CAP + 4000)
    probe.plant(**scene)
    v = probe.view(pose, K4, Z_MIN, ORG, CROP)
    m0 = _matches_for(rng, c.n, len(v["xy"]), c.nk, c.claim_all)
    if c.cull == "all":
        m0 = (m0[0][:0], m0[1][:0], m0[2][:0])
    c6 = probe.update(frames[0], wc, serial, MAX_AGE, c.max_obs, *m0)
    capacity = max(int(c6[5]) + c.delta, c.n0, 16)         # (a map that loses everything still has to hold what is planted)
    assert capacity <= KP_CAP and (c.cull == "all" or capacity == int(c6[5]) + c.delta), (c.name, capacity, tuple(c6))
    h = ctx.map_create(capacity)
    try:
        ref = M.MapRef(capacity, KP_CAP)
        _plant_both(ctx, h, ref, scene)
        figs = []
        for rnd, f in enumerate(frames):
            want_v = ref.view(pose, K4, Z_MIN, ORG, CROP)
            c2 = ctx.map_view(h, pose, K4, Z_MIN, REF_SLOT, VIEW_SLOT)
            assert tuple(c2) == tuple(want_v["counts2"]), "round %d: counts2 %s, want %s" % (rnd, tuple(c2), tuple(want_v["counts2"]))
            q, t, mask = m0 if rnd == 0 else _matches_for(rng, (c.n // 2, 0)[rnd - 1], len(want_v["xy"]), len(f["xy"]))
            ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
            s = serial + (0, 1, 5)[rnd]                       # (the third round ages a good part of the map out)
            want = ref.update(f, wc, s, MAX_AGE, c.max_obs, q, t, mask)
            got = ctx.map_update(h, NEW_SLOT, wc, s, MAX_AGE, c.max_obs, q, t, mask) if len(q) else ctx.map_update(h, NEW_SLOT, wc, s, MAX_AGE, c.max_obs)
            assert tuple(got) == tuple(want), "round %d: counts6 %s, want %s" % (rnd, tuple(got), tuple(want))
            _same_map(ctx, h, ref)
            figs.append([int(x) for x in got])
        want_v = ref.view(pose, K4, Z_MIN, ORG, CROP)
        _same_view(ctx, ctx.map_view(h, pose, K4, Z_MIN, REF_SLOT, VIEW_SLOT), want_v)
        print("%s: capacity %d, counts6 per round %s, final view %s" % (c.name, capacity, figs, tuple(want_v["counts2"])), flush=True)
        return dict(capacity=capacity, counts=figs)
    finally:
        ctx.map_destroy(h)


def _update_body():
    ctx = _context()
    out = {}
    for c in UPDATE_CASES:
        _guard(out, c.name, lambda: _update_case(ctx, c))
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---- refusals
REFUSALS = ("duplicate_q", "q_beyond_the_view", "t_beyond_the_slot", "decreasing_serial", "slot_without_depth", "view_into_ref_slot",
            "capacity_above_kp_cap", "fifth_map", "destroyed_handle", "null_pointers", "hostile_integers", "update_without_a_view")


def _refusal_body():
    import ctypes
    from openvo_amd import _native
    ctx = _context()
    lib, hnd = ctx._lib, ctx._h
    rng = np.random.default_rng(23)
    scene = _map_scene(200, rng, 20, 10)
    h = ctx.map_create(400)
    ctx.plant_map(h, **scene)
    pose, wc = pose_cw(), _inv34(pose_cw())
    f = _frame_for(rng, 60)
    ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
    n_view = int(ctx.map_view(h, pose, K4, Z_MIN, REF_SLOT, VIEW_SLOT)[1])
    assert n_view >= 150
    before = ctx.map_download(h)
    out = {}

    def refused(code, fn):
        def run():
            try:
                fn()
            except _native.VoError as e:
                assert e.code == code, "status %d, want %d (%s)" % (e.code, code, e)
            else:
                raise AssertionError("the call was not refused")
            after = ctx.map_download(h)
            for k in before:
                assert np.array_equal(_bits(before[k]) if k == "xyz" else before[k], _bits(after[k]) if k == "xyz" else after[k]), "%s changed" % k
        return run

    def raw(rc_fn, code):
        def run():
            rc = rc_fn()
            if rc != 0:
                raise _native.VoError(rc, "raw call")
        return refused(code, run)

    i32 = lambda *v: np.array(v, np.int32)                                           # noqa: E731
    up = lambda q, t, m, serial=20, slot=NEW_SLOT: ctx.map_update(h, slot, wc, serial, MAX_AGE, 8, i32(*q), i32(*t), np.array(m, np.uint8))   # noqa: E731
    _guard(out, "duplicate_q", refused(VO_E_ARG, lambda: up((3, 7, 3), (1, 2, 4), (1, 1, 1))))
    _guard(out, "q_beyond_the_view", refused(VO_E_ARG, lambda: up((0, n_view), (1, 2), (1, 0))))
    _guard(out, "t_beyond_the_slot", refused(VO_E_ARG, lambda: up((0, 1), (1, 60), (0, 1))))
    _guard(out, "decreasing_serial", refused(VO_E_ARG, lambda: up((0,), (1,), (1,), serial=int(scene["last"].max()) - 1)))
    _guard(out, "slot_without_depth", refused(VO_E_STATE, lambda: up((0,), (0,), (1,), slot=9)))
    _guard(out, "view_into_ref_slot", refused(VO_E_ARG, lambda: ctx.map_view(h, pose, K4, Z_MIN, REF_SLOT, REF_SLOT)))
    _guard(out, "capacity_above_kp_cap", refused(VO_E_ARG, lambda: ctx.map_create(KP_CAP + 1)))

    def fifth():
        hs = [ctx.map_create(16) for _ in range(3)]
        try:
            ctx.map_create(16)
        finally:
            for x in hs:
                ctx.map_destroy(x)
    _guard(out, "fifth_map", refused(VO_E_CAP, fifth))

    def destroyed():
        x = ctx.map_create(16)
        ctx.map_destroy(x)
        ctx.map_reset(x)
    _guard(out, "destroyed_handle", refused(VO_E_ARG, destroyed))

    def nulls():
        vp = ctypes.c_void_p
        Rt, k4, c2, c6 = np.ascontiguousarray(pose.reshape(12)), np.array(K4, np.float64), np.zeros(2, np.int32), np.zeros(6, np.int32)
        q = np.zeros(1, np.int32)
        p = lambda a: a.ctypes.data_as(vp)                                           # noqa: E731
        calls = [lambda: lib.vo_map_create(hnd, 16, None), lambda: lib.vo_map_create(None, 16, None), lambda: lib.vo_map_reset(None, h),
                 lambda: lib.vo_map_view(hnd, h, None, p(k4), Z_MIN, REF_SLOT, VIEW_SLOT, p(c2)),
                 lambda: lib.vo_map_view(hnd, h, p(Rt), None, Z_MIN, REF_SLOT, VIEW_SLOT, p(c2)),
                 lambda: lib.vo_map_view(hnd, h, p(Rt), p(k4), Z_MIN, REF_SLOT, VIEW_SLOT, None),
                 lambda: lib.vo_map_update(hnd, h, NEW_SLOT, None, 20, 5, 8, None, None, None, 0, p(c6)),
                 lambda: lib.vo_map_update(hnd, h, NEW_SLOT, p(Rt), 20, 5, 8, None, None, None, 0, None),
                 lambda: lib.vo_map_update(hnd, h, NEW_SLOT, p(Rt), 20, 5, 8, None, p(q), p(q), 1, p(c6)),
                 lambda: lib.vo_map_update(hnd, h, NEW_SLOT, p(Rt), 20, 5, 8, p(q), p(q), None, 1, p(c6)),
                 lambda: lib.vo_map_download(None, h, None, None, None, None, None, 0, None)]
        for k, call in enumerate(calls):
            rc = call()
            assert rc == VO_E_ARG, "null-pointer call %d returned %d" % (k, rc)
        raise _native.VoError(VO_E_ARG, "every null-pointer call was refused")
    _guard(out, "null_pointers", refused(VO_E_ARG, nulls))

    def hostile():
        vp = ctypes.c_void_p
        Rt, k4, c2, c6 = np.ascontiguousarray(pose.reshape(12)), np.array(K4, np.float64), np.zeros(2, np.int32), np.zeros(6, np.int32)
        q, m8, out = np.zeros(4, np.int32), np.ones(4, np.uint8), ctypes.c_int(0)
        p = lambda a: a.ctypes.data_as(vp)                                           # noqa: E731
        big, small = 2 ** 31 - 1, -2 ** 31
        calls = [lambda x=x: lib.vo_map_create(hnd, x, ctypes.byref(out)) for x in (small, -1, 0, 15, KP_CAP + 1, big)]
        for x in (small, -1, 1, 2, 3, 4, 1000, big):                                 # (handle 0 is the one map there is)
            calls += [lambda x=x: lib.vo_map_reset(hnd, x), lambda x=x: lib.vo_map_destroy(hnd, x),
                      lambda x=x: lib.vo_map_view(hnd, x, p(Rt), p(k4), Z_MIN, REF_SLOT, VIEW_SLOT, p(c2)),
                      lambda x=x: lib.vo_map_update(hnd, x, NEW_SLOT, p(Rt), 20, 5, 8, None, None, None, 0, p(c6)),
                      lambda x=x: lib.vo_map_download(hnd, x, None, None, None, None, None, 0, ctypes.byref(out))]
        for x in (small, -1, 28, 29, 1000, big):                                     # slots
            calls += [lambda x=x: lib.vo_map_view(hnd, h, p(Rt), p(k4), Z_MIN, x, VIEW_SLOT, p(c2)),
                      lambda x=x: lib.vo_map_view(hnd, h, p(Rt), p(k4), Z_MIN, REF_SLOT, x, p(c2)),
                      lambda x=x: lib.vo_map_update(hnd, h, x, p(Rt), 20, 5, 8, None, None, None, 0, p(c6))]
        for x in (small, -1, KP_CAP + 1, big):                                       # n
            calls.append(lambda x=x: lib.vo_map_update(hnd, h, NEW_SLOT, p(Rt), 20, 5, 8, p(q), p(q), p(m8), x, p(c6)))
        for age, obs, ser in ((-1, 8, 20), (small, 8, 20), (5, 0, 20), (5, -1, 20), (5, 65536, 20), (5, big, 20), (5, 8, -1), (5, 8, small)):
            calls.append(lambda a=age, o=obs, s_=ser: lib.vo_map_update(hnd, h, NEW_SLOT, p(Rt), s_, a, o, None, None, None, 0, p(c6)))
        for z in (-1.0, float("nan"), float("inf")):
            calls.append(lambda z=z: lib.vo_map_view(hnd, h, p(Rt), p(k4), z, REF_SLOT, VIEW_SLOT, p(c2)))
        bad_pose = Rt.copy(); bad_pose[7] = np.nan
        calls += [lambda: lib.vo_map_view(hnd, h, p(bad_pose), p(k4), Z_MIN, REF_SLOT, VIEW_SLOT, p(c2)),
                  lambda: lib.vo_map_update(hnd, h, NEW_SLOT, p(bad_pose), 20, 5, 8, None, None, None, 0, p(c6))]
        for k, call in enumerate(calls):
            rc = call()
            assert rc == VO_E_ARG, "hostile call %d returned %d" % (k, rc)
        # a download into too little room is the one capacity status
        assert lib.vo_map_download(hnd, h, p(np.zeros(3, np.float32)), None, None, None, None, 1, ctypes.byref(out)) == VO_E_CAP
        raise _native.VoError(VO_E_ARG, "every hostile call was refused")
    _guard(out, "hostile_integers", refused(VO_E_ARG, hostile))

    def no_view():
        tf = int(np.flatnonzero(np.isfinite(f["xyz"]).all(1))[0])
        assert tuple(up((0,), (tf,), (1,)))[0] == 1         # a good update: the map changes, the view is void from here on
        before.update(ctx.map_download(h))
        up((0,), (tf,), (1,), serial=21)
    _guard(out, "update_without_a_view", refused(VO_E_ARG, no_view))
    ctx.map_destroy(h)
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---------------------------------------------------------------------------------------------- in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_map as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("MAP-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("MAP-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("MAP-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", ["visible%d" % V for V in VIEW_COUNTS] + ["exact_edges"])
def test_view_equals_the_restatement_and_feeds_the_pnp_step(name):
    res = _child("_view_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", [c.name for c in UPDATE_CASES])
def test_update_equals_the_restatement(name):
    res = _child("_update_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_leave_the_map_unchanged(name):
    res = _child("_refusal_body()")[name]
    assert res["ok"], res["err"]


# ---- the odometer (the product library, in this process)
def _chain(odo, frames):
    return [(odo.update(L, R), odo.skip_cause, odo.skipped_frames, getattr(odo, "track_source", None), odo.c_T_w.copy()) for L, R in frames]


@pytest.fixture(scope="module")
def c1():
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    ctx = _native.Context(0, 640, 480, 64, 500)
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)
    yield dict(ctx=ctx, cam=cam, frames=c.pairs(0, 8), cache={})
    ctx.close()


BASE = dict(preprocessed_frames=True, depth="sparse", pose_method="pnp")


@pytest.mark.parametrize("name,kw", [("default", {}), ("cross-window", dict(cross_check=True, match_window=(24, 16)))])
def test_map_odometer_equals_the_cpu_chain(oracle, c1, name, kw):
    """C1 frames 0-7, 500 features: accept flags, skip_cause, skipped_frames, track_source and the counts of every view and update
    equal the CPU chain (MapRefOdometer on the oracle's ORB), c_T_w to 1e-9; landmark descriptors, obs and last exactly, positions
    to 1e-5 m (float32 of poses that agree to 1e-9); run() equals update(); track="pair" before and after equals the pairwise
    chain.  cross-window: the cross-check and a match window (a guided search around the predicted pixel) compose unchanged."""
    import sparse_stereo_ref as S
    from openvo_amd import StereoOdometer
    from openvo_amd.synth import Corridor
    cam, frames, cache = c1["cam"], c1["frames"], c1["cache"]
    kw = dict(BASE, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("cross_check", "match_window")}
    pair_want = _chain(S.SparseRefOdometer(oracle, cam.Q, cam.valid_region_left, frames=cache, pose_method="pnp", **ref_kw), frames)
    before = _chain(StereoOdometer(cam, **kw), frames)
    ref = M.MapRefOdometer(oracle, cam.Q, cam.valid_region_left, frames=cache, **ref_kw)
    want, want_counts = [], []
    for L, R in frames:
        want.append((ref.update(L, R), ref.skip_cause, ref.skipped_frames, ref.track_source, ref.c_T_w.copy()))
        want_counts.append({k: tuple(int(x) for x in v) for k, v in ref.map_counts.items()})
    odo = StereoOdometer(cam, track="map", **kw)
    assert odo.landmarks()["xyz"].shape == (0, 3)
    got, got_counts = [], []
    for L, R in frames:
        got.append((odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.track_source, odo.c_T_w.copy()))
        got_counts.append({k: tuple(int(x) for x in v) for k, v in odo.map_counts.items()})
    assert [w[0] for w in want] == [True] * 8 and want[0][3] is None and [w[3] for w in want[1:]].count("map") >= 6, [w[:4] for w in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:4] == w[:4], (k, g[:4], w[:4])
        assert np.allclose(g[4], w[4], rtol=0, atol=1e-9), (k, np.abs(g[4] - w[4]).max())
        assert got_counts[k] == want_counts[k], (k, got_counts[k], want_counts[k])
    lm, wm = odo.landmarks(), ref.map.download()
    assert len(lm["xyz"]) == len(wm["xyz"]) == want_counts[-1]["update"][5] > 500
    for k in ("desc", "octave", "obs", "last"):
        assert np.array_equal(lm[k], wm[k]), k
    assert np.abs(lm["xyz"] - wm["xyz"]).max() <= 1e-5
    assert lm["obs"].max() >= 4
    view_slot = odo._view_slot
    assert view_slot is not None and cam._slot_owner[view_slot] is not None
    odo2 = StereoOdometer(cam, track="map", **kw)
    ran = [(ok, odo2.skip_cause, odo2.skipped_frames, odo2.track_source, odo2.c_T_w.copy()) for ok in odo2.run(iter(frames), depth=4)]
    for g, r in zip(got, ran):
        assert g[:4] == r[:4] and np.array_equal(g[4], r[4])
    odo.release_map()
    odo2.release_map()
    assert cam._slot_owner[view_slot] is None
    after = _chain(StereoOdometer(cam, **kw), frames)
    for b, a, w in zip(before, after, pair_want):
        assert b[:3] == a[:3] == w[:3] and np.array_equal(b[4], a[4]) and np.allclose(b[4], w[4], rtol=0, atol=1e-9)
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(frames) - 1)
    print("%s: end-point error over 7 pairs: pairwise %.3f m, map %.3f m; map of %d landmarks; placed by %s" % (
        name, np.linalg.norm(np.linalg.inv(before[-1][4])[:3, 3] - gt[:3, 3]), np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3]), len(lm["xyz"]),
        [g[3] for g in got]))


def test_map_odometer_loop_check_refine_and_seams(c1):
    """loop_check composes through the landmarks' right descriptors: a threshold of 256 gives the chain without it, bit for bit, and
    at 48 bits the map step still places every frame (it could not with anything but the partners' real descriptors in the view);
    pnp_refine composes (the gates see the refined pose); where the fused step cannot run there is no map mode."""
    from openvo_amd import StereoOdometer
    cam, frames = c1["cam"], c1["frames"]
    chains = {}
    for name, kw in (("plain", {}), ("loop256", dict(loop_check=256)), ("loop48", dict(loop_check=48)), ("refine3", dict(pnp_refine=3))):
        odo = StereoOdometer(cam, track="map", **dict(BASE, **kw))
        chains[name] = (_chain(odo, frames), odo.map_counts["update"].copy(), odo.landmarks())
        odo.release_map()
    for g, w in zip(chains["loop256"][0], chains["plain"][0]):
        assert g[:4] == w[:4] and np.array_equal(g[4], w[4])
    assert np.array_equal(chains["loop256"][1], chains["plain"][1])
    for k in ("xyz", "desc", "obs", "last"):
        assert np.array_equal(chains["loop256"][2][k], chains["plain"][2][k]), k
    for name in ("loop48", "refine3"):
        assert [g[0] for g in chains[name][0]] == [True] * 8 and [g[3] for g in chains[name][0]] == [None] + ["map"] * 7, (name, [g[:4] for g in chains[name][0]])
    assert 0 < chains["loop48"][1][0] <= chains["plain"][1][0]              # observed: the loop check only ever removes matches
    assert not np.array_equal(chains["refine3"][0][-1][4], chains["plain"][0][-1][4])
    # the bar tests/test_sparse_stereo_ref.py holds the sparse PnP chain to over these eight frames: a fifth of the dense default's 1.303 m
    from openvo_amd.synth import Corridor
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(frames) - 1)
    for name in ("plain", "loop48", "refine3"):
        e = float(np.linalg.norm(np.linalg.inv(chains[name][0][-1][4])[:3, 3] - gt[:3, 3]))
        print("%s: end-point error %.3f m" % (name, e))
        assert e <= 1.303 / 5, (name, e)
    odo3 = StereoOdometer(cam, track="map", **BASE)
    odo3.point_clouds = odo3.point_clouds
    with pytest.raises(ValueError, match="track='map'"):
        odo3.update(*frames[0])
