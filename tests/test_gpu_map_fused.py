"""The fused map step on the GPU (csrc/map.hip: vo_track_map = k_map_view_pad -> kNN-2 -> the PnP chain -> k_map_decide ->
k_map_update_dev, one synchronisation) against the unfused chain on a twin map in the same context (vo_map_view + vo_pnp_pair + the
host's decisions + vo_map_update) and against the numpy restatement (tests/map_fused_ref.py), with maps and keypoints PLANTED
through the test-only library as tests/test_gpu_map.py does (whose scenes and helpers this file borrows):

    padded view   maps of 63, 64, 65, 1023, 1024, 1025 landmarks (under / at / above a wave and a trip of the 1024-thread workgroup)
                  with an invisible subset that holds the first landmark, the last one and the last landmark of a trip: rows
                  [0, vis) and view_src equal vo_map_view's on the twin bit for bit, the padding behind them is row 0's clone with
                  a NaN point, the slot's count is vis afterwards; one map of which nothing is visible (zero padding).
    step          plain, cross_check, a window, the loop check, pnp_refine=3: the record, q / t / mask and all six counts equal the
                  unfused chain's exactly; the map afterwards equals it in obs / last / octave / desc, and in xyz bit for bit
                  against the restatement and within 2 float32 ulps of the unfused map (np.linalg.inv against the rigid inverse).
                  The cross_check case plants invisible landmarks that ARE the nearest query of a train descriptor.
    decisions     one planted input per code; after every refusal the map is byte-identical and a vo_map_view on it works.
    refusals      every bad argument its status, the map unchanged; a map of 3801 landmarks is VO_E_CAP.
    odometer      StereoOdometer(track="map", map_fused=True) on C1 frames 0-7 against MapFusedRefOdometer.

The planted cases run in one child process per group, VO355_LIB pointing at the test-only library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_fused_ref as F                  # noqa: E402
import map_ref as M                        # noqa: E402
import planted as P                        # noqa: E402
import test_gpu_map as G                   # noqa: E402  (scenes, the context, the comparisons: nothing of it is collected from here)

pytestmark = pytest.mark.gpu

ROOT = G.ROOT
K4, Z_MIN, ORG, CROP, KP_CAP = G.K4, G.Z_MIN, G.ORG, G.CROP, G.KP_CAP
RATIO, ITERS, THR, SEED = G.RATIO, G.ITERS, G.THR, G.SEED
VIEW_SLOT, VIEW2, NEW_SLOT = 3, 4, 5       # the fused step's view, the twin's view, the new frame (it holds the image)
MAX_AGE, MAX_OBS, SERIAL = 5, 8, 20
MAXD, MAXR = 1.0, np.pi / 3
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
PAD_SIZES = (63, 64, 65, 1023, 1024, 1025)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- scenes
def map_scene(n, rng, invisible=()):
    """n landmarks inside the crop under G.pose_cw(), those named in `invisible` behind the camera, outside the image or not finite"""
    Xc = G._cam_point(rng.uniform(2, CROP[0] - 3, n), rng.uniform(2, CROP[1] - 3, n), rng.uniform(1.0, 12.0, n)).reshape(n, 3)
    xyz = G._to_world(Xc)
    for k, i in enumerate(invisible):
        kind = k % 4
        if kind == 0:
            xyz[i] = G._to_world(G._cam_point(np.array([300.0]), np.array([200.0]), -3.0))[0]          # behind the camera
        elif kind == 1:
            xyz[i] = G._to_world(G._cam_point(np.array([CROP[0] + 200.0]), np.array([100.0]), 4.0))[0]  # right of the crop
        elif kind == 2:
            xyz[i] = (np.nan, 0, 3)
        else:
            xyz[i] = G._to_world(G._cam_point(np.array([100.0]), np.array([-150.0]), 5.0))[0]           # above the crop
    return dict(xyz=xyz.astype(np.float32), desc=G._descs(n, rng), rdesc=G._descs(n, rng), octave=rng.integers(0, 8, n).astype(np.int32),
                obs=rng.integers(1, 12, n).astype(np.int32), last=rng.integers(SERIAL - MAX_AGE, SERIAL, n).astype(np.int32))


def pad_invisible(n, rng):
    """the first landmark, the last one, the last of a trip (1023, where there is one) and one in six of the others"""
    inv = {0, n - 1} | ({1023} if n > 1023 else set()) | set(int(i) for i in np.flatnonzero(rng.random(n) < 1 / 6))
    return sorted(inv)


def new_frame(view, rng, M_want, extra=7, noise=0.3, at_projection=0.7, loop_bits=None):
    """G.new_frame with the matches returned too: M of the view's keypoints seen again (descriptors with up to two bits flipped) from
    a camera moved by planted._motion().  loop_bits: the right descriptors of the matched keypoints are the landmarks' with up to that
    many bits flipped (the others are random: they fail any loop check)"""
    V = len(view["xy"])
    Mw = min(V, M_want)
    nt = max(Mw + extra, 2)
    desc, rdesc = G._descs(nt, rng), G._descs(nt, rng)
    q = np.sort(rng.choice(V, Mw, replace=False)) if Mw else np.zeros(0, np.int64)
    t = rng.permutation(nt)[:Mw]
    R, tv = P._motion()
    xy = np.stack([rng.uniform(0, CROP[0], nt), rng.uniform(0, CROP[1], nt)], 1)
    xyz = P._cloud(nt, rng)
    for k in range(Mw):
        desc[t[k]] = view["desc"][q[k]]
        for bit in rng.choice(256, int(rng.integers(0, 3)), replace=False):
            desc[t[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
        if loop_bits is not None:
            rdesc[t[k]] = view["rdesc"][q[k]]
            for bit in rng.choice(256, int(rng.integers(0, loop_bits + 1)), replace=False):
                rdesc[t[k], bit >> 3] ^= np.uint8(1 << (bit & 7))
        Y = R @ view["xyz"][q[k]].astype(np.float64) + tv
        xyz[t[k]] = Y + rng.normal(0, 1e-3, 3)
        if rng.random() < at_projection:
            xy[t[k]] = [K4[0] * Y[0] / Y[2] + K4[2] - ORG[0] + noise * rng.normal(), K4[1] * Y[1] / Y[2] + K4[3] - ORG[1] + noise * rng.normal()]
    return dict(xy=xy.astype(np.float32), desc=desc, xyz=xyz.astype(np.float32), rdesc=rdesc, octave=np.zeros(nt, np.int32), q=q, t=t)


def random_frame(rng, nt=40):
    return dict(xy=np.stack([rng.uniform(0, CROP[0], nt), rng.uniform(0, CROP[1], nt)], 1).astype(np.float32), desc=G._descs(nt, rng),
                xyz=P._cloud(nt, rng).astype(np.float32), rdesc=G._descs(nt, rng), octave=np.zeros(nt, np.int32))


# ---------------------------------------------------------------------------------------------- in the child process
def _plant(ctx, handles, ref, s):
    for h in handles:
        ctx.plant_map(h, s["xyz"], s["desc"], s["rdesc"], s["octave"], s["obs"], s["last"])
    if ref is not None:
        ref.plant(s["xyz"], s["desc"], s["rdesc"], s["octave"], s["obs"], s["last"])


def _track(ctx, h, pose, min_matches=10, max_dist=MAXD, max_rot=MAXR, serial=SERIAL, refine=0, **kw):
    return ctx.map_track(h, NEW_SLOT, VIEW_SLOT, pose, K4, Z_MIN, RATIO, ITERS, THR, SEED, refine, min_matches, max_dist, max_rot, serial,
                         MAX_AGE, MAX_OBS, **kw)


def _same_download(a, b, what):
    assert len(a["xyz"]) == len(b["xyz"]), "%s: %d landmarks against %d" % (what, len(a["xyz"]), len(b["xyz"]))
    assert np.array_equal(_bits(a["xyz"]), _bits(b["xyz"])), "%s: xyz differs in %d places" % (what, int((_bits(a["xyz"]) != _bits(b["xyz"])).any(1).sum()))
    for k in ("desc", "octave", "obs", "last"):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---- padded view
def _pad_case(ctx, n, nothing=False):
    rng = np.random.default_rng([29, n, int(nothing)])
    inv = list(range(n)) if nothing else pad_invisible(n, rng)
    scene = map_scene(n, rng, inv)
    h, h2 = ctx.map_create(max(n, 16)), ctx.map_create(max(n, 16))
    try:
        ref = M.MapRef(max(n, 16), KP_CAP)
        _plant(ctx, (h, h2), ref, scene)
        pose = G.pose_cw()
        want = F.padded_view(ref, pose, K4, Z_MIN, ORG, CROP)
        vis = want["vis"]
        assert vis == n - len(inv), "the scene has %d visible landmarks, planned %d" % (vis, n - len(inv))
        c2 = ctx.map_view(h2, pose, K4, Z_MIN, NEW_SLOT, VIEW2)
        assert tuple(c2) == (n, vis)
        twin = dict(ctx.download_keypoints(VIEW2), xyz=ctx.download_keypoint_depth(VIEW2)[0], rdesc=ctx.download_keypoint_rdesc(VIEW2),
                    src=ctx.peek_view(h2, VIEW2, n)["src"][:vis])
        f = random_frame(rng)
        ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        before = ctx.map_download(h)
        r = _track(ctx, h, pose)
        assert tuple(r["view"]) == (n, vis), "view counts %s, want %s" % (tuple(r["view"]), (n, vis))
        assert r["decision"] in (1, 2), "a frame of random descriptors was not refused for its view or its matches: %d" % r["decision"]
        _same_download(ctx.map_download(h), before, "a refused step")
        # the slot stands as vo_map_view leaves it ...
        G._same_view(ctx, (n, vis), dict(want, xy=want["xy"][:vis], xyz=want["xyz"][:vis], desc=want["desc"][:vis], rdesc=want["rdesc"][:vis],
                                         octave=want["octave"][:vis]), slot=VIEW_SLOT)
        got = ctx.peek_view(h, VIEW_SLOT, n)
        # ... its rows and view_src are the twin's, bit for bit ...
        for k in ("xy", "xyz"):
            assert np.array_equal(_bits(got[k][:vis]), _bits(twin[k])), "%s of the view differs from vo_map_view's" % k
        for k in ("desc", "rdesc", "octave", "src"):
            assert np.array_equal(got[k][:vis], twin[k]), "%s of the view differs from vo_map_view's" % k
        assert np.array_equal(got["src"][:vis], want["src"])
        # ... and the padding is the restatement's
        assert np.isnan(got["xyz"][vis:]).all(), "padding kp_xyz is not NaN"
        assert np.array_equal(_bits(got["xy"][vis:]), _bits(want["xy"][vis:])), "padding kp_xy is not row 0's"
        for k in ("desc", "rdesc", "octave"):
            assert np.array_equal(got[k][vis:], want[k][vis:]), "padding %s is not row 0's" % k
        if nothing:
            assert vis == 0 and not got["xy"].any() and not got["desc"].any() and not got["rdesc"].any() and not got["octave"].any()
        print("pad n=%d: %d visible, %d padding rows, decision %d" % (n, vis, n - vis, r["decision"]), flush=True)
        return dict(n=n, vis=vis)
    finally:
        ctx.map_destroy(h)
        ctx.map_destroy(h2)


def _pad_body():
    ctx = G._context()
    out = {}
    for n in PAD_SIZES:
        G._guard(out, "n%d" % n, lambda: _pad_case(ctx, n))
    G._guard(out, "nothing_visible", lambda: _pad_case(ctx, 64, nothing=True))
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---- the step against the unfused chain
STEP_MODES = {
    "plain": dict(),
    "cross_check": dict(cross_check=True),
    "window": dict(window=(60.0, 45.0)),
    "loop": dict(loop=24),
    "refine3": dict(refine=3),
}
STEP_N, STEP_M = 1500, 400


def _host_decision(r, vis, min_matches=10, max_dist=MAXD, max_rot=MAXR):
    T = r["Rt_refined"] if r["refine_status"] == 0 else r["Rt"]
    return F.decide(vis, r["matches"], r["flags"], r["n"], r["best_count"], T, min_matches, max_dist, max_rot), T


def _step_case(ctx, name):
    kw = dict(STEP_MODES[name])
    refine = kw.pop("refine", 0)
    rng = np.random.default_rng([31, sorted(STEP_MODES).index(name)])
    inv = pad_invisible(STEP_N, rng)
    scene = map_scene(STEP_N, rng, inv)
    pose = G.pose_cw()
    probe = M.MapRef(STEP_N, KP_CAP)
    _plant(ctx, (), probe, scene)
    view = probe.view(pose, K4, Z_MIN, ORG, CROP)
    f = new_frame(view, rng, STEP_M, loop_bits=6 if name == "loop" else None)
    stolen = 0
    if name == "cross_check":
        # invisible landmarks whose descriptor IS a train descriptor that a visible landmark matches: in the compacted view they do
        # not exist; a padding that let dead rows into the column minima would take those matches away
        for i, k in zip(inv[2:40], range(0, 2 * 38, 2)):
            scene["desc"][i] = f["desc"][f["t"][k]]
            stolen += 1
    h, h2 = ctx.map_create(STEP_N + 600), ctx.map_create(STEP_N + 600)
    try:
        ref = M.MapRef(STEP_N + 600, KP_CAP)
        _plant(ctx, (h, h2), ref, scene)
        ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        # the unfused chain on the twin, composed here
        c2 = ctx.map_view(h2, pose, K4, Z_MIN, NEW_SLOT, VIEW2)
        vis = int(c2[1])
        u = ctx.pnp_pair_window(VIEW2, NEW_SLOT, RATIO, K4, kw.get("window"), ITERS, THR, SEED, refine, True, kw.get("cross_check", False), kw.get("loop"))
        dec, T = _host_decision(u, vis)
        assert dec == 0 and u["matches"] >= STEP_M // 2, "the unfused chain does not accept the planted frame: decision %d, M %d" % (dec, u["matches"])
        if name == "refine3":
            assert u["refine_status"] == 0 and u["refine_steps"] == 3
        cw_host = np.vstack([T, [0, 0, 0, 1]]) @ np.vstack([pose, [0, 0, 0, 1]])
        c6 = ctx.map_update(h2, NEW_SLOT, np.linalg.inv(cw_host), SERIAL, MAX_AGE, MAX_OBS, u["q"], u["t"], u["mask"])
        # the fused step
        r = _track(ctx, h, pose, refine=refine, **kw)
        assert r["decision"] == 0 and tuple(r["view"]) == tuple(c2) and r["update_flags"] == 0, (r["decision"], tuple(r["view"]), tuple(c2))
        for k in ("matches", "n", "best_iter", "best_count", "flags", "refine_status", "refine_steps"):
            assert r[k] == u[k], "%s: fused %d, unfused %d" % (k, r[k], u[k])
        for k in ("q", "t", "mask"):
            assert np.array_equal(r[k], u[k]), "%s differs from the unfused step's" % k
        assert np.array_equal(r["Rt"], u["Rt"]) and np.array_equal(r["Rt_refined"], u["Rt_refined"]), "the poses differ from the unfused step's"
        assert tuple(r["update"]) == tuple(c6), "counts6 %s, unfused %s" % (tuple(r["update"]), tuple(c6))
        assert np.abs(np.vstack([r["c_T_w"], [0, 0, 0, 1]]) - cw_host).max() <= 1e-12
        got, twin = ctx.map_download(h), ctx.map_download(h2)
        for k in ("desc", "octave", "obs", "last"):
            assert np.array_equal(got[k], twin[k]), "%s of the map differs from the unfused chain's" % k
        fin = np.isfinite(twin["xyz"])                        # (the planted landmarks without a finite position stay what they are)
        assert np.array_equal(_bits(got["xyz"])[~fin], _bits(twin["xyz"])[~fin]) and fin.sum() > 3 * STEP_N - 3 * len(inv)
        ulps = np.abs(got["xyz"][fin].astype(np.float64) - twin["xyz"][fin].astype(np.float64)) / np.spacing(np.abs(twin["xyz"][fin]))
        assert ulps.max() <= 2, "xyz is %.1f ulps from the unfused map's" % ulps.max()
        # the restatement, fed the step's own PnP record: the view, the decision, the composed pose, its inverse and the update
        want = F.track(ref, f, pose, K4, Z_MIN, ORG, CROP, lambda v, fr: {k: r[k] for k in ("matches", "flags", "n", "best_count", "Rt", "Rt_refined",
                                                                                              "refine_status", "q", "t", "mask")},
                       10, MAXD, MAXR, SERIAL, MAX_AGE, MAX_OBS)
        assert want["decision"] == 0 and tuple(want["update"]) == tuple(r["update"])
        assert np.array_equal(want["c_T_w"], r["c_T_w"]) and np.array_equal(want["w_T_c"], r["w_T_c"]), "c_T_w / w_T_c are not the restatement's bit for bit"
        G._same_map(ctx, h, ref)
        # what follows works on the map the step left: a view of it, and the step again
        G._same_view(ctx, ctx.map_view(h, pose, K4, Z_MIN, NEW_SLOT, VIEW_SLOT), ref.view(pose, K4, Z_MIN, ORG, CROP), slot=VIEW_SLOT)
        fig = dict(vis=vis, M=r["matches"], n=r["n"], best_count=r["best_count"], counts6=[int(x) for x in c6], xyz_ulps=float(ulps.max()),
                   moved=int((_bits(got["xyz"]) != _bits(twin["xyz"])).any(1).sum()), stolen=stolen)
        print("%s: %s" % (name, fig), flush=True)
        return fig
    finally:
        ctx.map_destroy(h)
        ctx.map_destroy(h2)


def _step_body():
    ctx = G._context()
    out = {}
    for name in STEP_MODES:
        G._guard(out, name, lambda: _step_case(ctx, name))
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---- decisions
DECISIONS = {     # name: (code, scene / frame variant, the step's arguments)
    "0_accepted": (0, "good", {}),
    "1_view": (1, "few_visible", {}),
    "2_matches": (2, "random_frame", {}),
    "3_usable": (3, "three_matches", dict(min_matches=2)),
    "4_outlier": (4, "scattered", {}),
    "6_bigdist": (6, "good", dict(max_dist=0.25)),
    "7_bigrot": (7, "good", dict(max_rot=0.03)),
    "7_both_gates": (7, "good", dict(max_dist=0.25, max_rot=0.03)),
}
FAULT_DECISIONS = {"5_nan": ("VO_FAULT_MAP_NAN", 5), "8_index": ("VO_FAULT_PNP_RANGE", 8)}
DEC_N = 300


def _decision_scene(variant, rng):
    inv = pad_invisible(DEC_N, rng) if variant != "few_visible" else list(range(5, DEC_N))
    scene = map_scene(DEC_N, rng, inv)
    probe = M.MapRef(DEC_N + 200, KP_CAP)
    _plant(None, (), probe, scene)
    view = probe.view(G.pose_cw(), K4, Z_MIN, ORG, CROP)
    if variant == "random_frame":
        f = random_frame(rng, 150)
    elif variant == "three_matches":
        f = new_frame(view, rng, 3, extra=60, at_projection=1.0)
    elif variant == "scattered":
        f = new_frame(view, rng, 120, at_projection=0.0)
    else:
        f = new_frame(view, rng, 120)
    return scene, f


def _after_refusal(ctx, h, before, ref):
    _same_download(ctx.map_download(h), before, "after the refusal")
    G._same_view(ctx, ctx.map_view(h, G.pose_cw(), K4, Z_MIN, NEW_SLOT, VIEW_SLOT), ref.view(G.pose_cw(), K4, Z_MIN, ORG, CROP), slot=VIEW_SLOT)


def _decision_case(ctx, name):
    code, variant, args = DECISIONS[name]
    rng = np.random.default_rng([37, sorted(DECISIONS).index(name)])
    scene, f = _decision_scene(variant, rng)
    pose = G.pose_cw()
    h, h2 = ctx.map_create(DEC_N + 200), ctx.map_create(DEC_N + 200)
    try:
        ref = M.MapRef(DEC_N + 200, KP_CAP)
        _plant(ctx, (h, h2), ref, scene)
        ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        vis = int(ctx.map_view(h2, pose, K4, Z_MIN, NEW_SLOT, VIEW2)[1])
        u = ctx.pnp_pair(VIEW2, NEW_SLOT, RATIO, K4, ITERS, THR, SEED, 0, True)
        mm, md, mr = args.get("min_matches", 10), args.get("max_dist", MAXD), args.get("max_rot", MAXR)
        want, T = _host_decision(u, vis, mm, md, mr)
        assert want == code, "the planted input is decided %d by the host's chain, planned %d (vis %d, M %d, n %d, inliers %d)" % (
            want, code, vis, u["matches"], u["n"], u["best_count"])
        fig = dict(vis=vis, M=u["matches"], n=u["n"], best_count=u["best_count"])
        if code in (0, 6, 7):
            dist, angle = F.gate_figures(T)
            assert abs(dist - md) > 1e-6 * md and abs(angle - mr) > 1e-6 * mr, "a gated pose within 1e-6 of its gate: %r %r" % (dist, angle)
            assert (dist > md, angle > mr) == {"0_accepted": (False, False), "6_bigdist": (True, False), "7_bigrot": (False, True),
                                               "7_both_gates": (True, True)}[name]
            fig.update(dist=dist, angle=angle)
        before = ctx.map_download(h)
        r = _track(ctx, h, pose, **args)
        assert r["decision"] == code, "decision %d, want %d" % (r["decision"], code)
        assert tuple(r["view"]) == (DEC_N, vis)
        if code == 0:
            assert r["update"][5] == len(ctx.map_download(h)["xyz"]) > 0 and (r["update"] >= 0).all()
        else:
            assert list(r["update"]) == [-1] * 6 and not r["c_T_w"].any() and not r["w_T_c"].any()
            _after_refusal(ctx, h, before, ref)
        print("%s: %s" % (name, fig), flush=True)
        return fig
    finally:
        ctx.map_destroy(h)
        ctx.map_destroy(h2)


def _decision_body():
    ctx = G._context()
    out = {}
    for name in DECISIONS:
        G._guard(out, name, lambda: _decision_case(ctx, name))
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


def _fault_body(name):
    """decisions 5 and 8: the test-only library's fault hooks make the FIRST step of this process hand on a NaN pose entry / hold its
    match indices to a train set of one descriptor (the environment variable is set by the parent)"""
    from openvo_amd import _native
    code = FAULT_DECISIONS[name][1]
    ctx = G._context()
    out = {}

    def run():
        rng = np.random.default_rng([41, code])
        scene, f = _decision_scene("good", rng)
        h = ctx.map_create(DEC_N + 200)
        ref = M.MapRef(DEC_N + 200, KP_CAP)
        _plant(ctx, (h,), ref, scene)
        ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        before = ctx.map_download(h)
        if code == 8:
            try:
                _track(ctx, h, G.pose_cw())
            except _native.VoError as e:
                assert e.code == VO_E_STATE, "status %d, want VO_E_STATE" % e.code
            else:
                raise AssertionError("an index outside the train set was not refused")
        else:
            r = _track(ctx, h, G.pose_cw())
            assert r["decision"] == 5 and list(r["update"]) == [-1] * 6, (r["decision"], list(r["update"]))
            assert r["best_count"] >= 10 and not np.isnan(r["Rt"]).any()          # (the PnP step itself was healthy)
        _after_refusal(ctx, h, before, ref)
        r = _track(ctx, h, G.pose_cw())                                            # the fault is spent: the same input is accepted
        assert r["decision"] == 0, r["decision"]
        ctx.map_destroy(h)
    G._guard(out, name, run)
    ctx.close()
    print("MAP-RESULT " + json.dumps(out))


# ---- refusals
REFUSALS = ("view_into_the_new_slot", "hostile_slots_and_handles", "null_pointers", "bad_pose_K4_z_min", "bad_match_flags", "bad_pnp_arguments",
            "bad_gates_and_min_matches", "bad_update_arguments", "decreasing_serial", "slot_without_an_image", "slot_without_depth",
            "train_set_of_one", "outputs_too_small", "map_above_3800")


def _refusal_body():
    import ctypes
    from openvo_amd import _native
    ctx = G._context()
    lib, hnd = ctx._lib, ctx._h
    rng = np.random.default_rng(43)
    scene, f = _decision_scene("good", rng)
    h = ctx.map_create(DEC_N + 200)
    ctx.plant_map(h, **scene)
    ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
    blank = np.zeros((G.H, G.W), np.uint8)
    ctx.upload_pair(7, blank, blank, True)                    # an image, no keypoints
    before = ctx.map_download(h)
    out = {}
    vp = ctypes.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)                        # noqa: E731
    pose12, k4 = np.ascontiguousarray(G.pose_cw().reshape(12)), np.array(K4, np.float64)
    rec = _native.MapTrackRec()
    arrs = [np.zeros(KP_CAP, np.uint8), np.zeros(KP_CAP, np.int32), np.zeros(KP_CAP, np.int32)]
    good = dict(map=h, slot_new=NEW_SLOT, view_slot=VIEW_SLOT, pose=pose12, K4=k4, z_min=Z_MIN, ratio=RATIO, flags=0, iters=ITERS, thr=THR, seed=SEED,
                refine=0, min_matches=10, max_dist=MAXD, max_rot=MAXR, serial=SERIAL, max_age=MAX_AGE, max_obs=MAX_OBS, rec=ctypes.byref(rec),
                mask=None, q=None, t=None, cap=0)

    def raw(**change):
        a = dict(good, **change)
        return lib.vo_track_map(hnd, a["map"], a["slot_new"], a["view_slot"], p(a["pose"]), p(a["K4"]), a["z_min"], a["ratio"], a["flags"], a["iters"],
                                a["thr"], a["seed"], a["refine"], a["min_matches"], a["max_dist"], a["max_rot"], a["serial"], a["max_age"],
                                a["max_obs"], a["rec"], p(a["mask"]), p(a["q"]), p(a["t"]), a["cap"])

    def refused(code, changes, handle=h, kept=before):
        def run():
            for k, change in enumerate(changes):
                rc = raw(**change)
                assert rc == code, "call %d (%s) returned %d, want %d: %s" % (k, sorted(change), rc, code, ctx._lib.vo_last_error(hnd))
            _same_download(ctx.map_download(handle), kept, "after the refusals")
            return dict(calls=len(changes))
        return run

    big, small = 2 ** 31 - 1, -2 ** 31
    bad_pose, bad_k = pose12.copy(), k4.copy()
    bad_pose[7] = np.nan
    bad_k[2] = np.inf
    G._guard(out, "view_into_the_new_slot", refused(VO_E_ARG, [dict(view_slot=NEW_SLOT)]))
    G._guard(out, "hostile_slots_and_handles", refused(VO_E_ARG, [dict(slot_new=x) for x in (small, -1, 28, 1000, big)] + [dict(view_slot=x) for x in (small, -1, 28, big)]
                                                       + [dict(map=x) for x in (small, -1, 1, 3, 4, big)]))
    G._guard(out, "null_pointers", refused(VO_E_ARG, [dict(pose=None), dict(K4=None), dict(rec=None)]))
    G._guard(out, "bad_pose_K4_z_min", refused(VO_E_ARG, [dict(pose=bad_pose), dict(K4=bad_k), dict(K4=np.array([0.0, 500, 352, 256])), dict(K4=np.array([500.0, -1, 352, 256])),
                                                          dict(z_min=-1.0), dict(z_min=float("nan")), dict(z_min=float("inf"))]))
    # (no window and no loop threshold has been set in this context)
    G._guard(out, "bad_match_flags", refused(VO_E_ARG, [dict(flags=8), dict(flags=-1), dict(flags=_native.VO_MATCH_WINDOW), dict(flags=_native.VO_MATCH_LOOP)]))
    G._guard(out, "bad_pnp_arguments", refused(VO_E_ARG, [dict(iters=0), dict(iters=-5), dict(iters=(1 << 22) + 1), dict(refine=-1), dict(refine=21), dict(thr=0.0),
                                                          dict(thr=float("nan"))]))
    G._guard(out, "bad_gates_and_min_matches", refused(VO_E_ARG, [dict(min_matches=-1), dict(min_matches=small), dict(max_dist=float("nan")), dict(max_rot=float("nan"))]))
    G._guard(out, "bad_update_arguments", refused(VO_E_ARG, [dict(max_age=-1), dict(max_age=small), dict(max_obs=0), dict(max_obs=-1), dict(max_obs=65536), dict(max_obs=big)]))
    G._guard(out, "decreasing_serial", refused(VO_E_ARG, [dict(serial=int(scene["last"].max()) - 1), dict(serial=-1), dict(serial=small)]))
    G._guard(out, "slot_without_an_image", refused(VO_E_STATE, [dict(slot_new=9)]))
    G._guard(out, "slot_without_depth", refused(VO_E_STATE, [dict(slot_new=7)]))

    def one_train():
        ctx.plant_keypoints(NEW_SLOT, f["xy"][:1], f["desc"][:1], f["xyz"][:1], f["rdesc"][:1])
        try:
            return refused(VO_E_ARG, [dict()])()
        finally:
            ctx.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
    G._guard(out, "train_set_of_one", one_train)
    G._guard(out, "outputs_too_small", refused(VO_E_CAP, [dict(mask=arrs[0], cap=DEC_N - 1), dict(q=arrs[1], cap=0), dict(t=arrs[2], cap=-1)]))
    # every refusal above left the step possible: it is accepted now, and with arrays of exactly the map's size
    rc = raw(mask=arrs[0], q=arrs[1], t=arrs[2], cap=DEC_N)
    assert rc == 0 and rec.decision == 0 and rec.counts6[5] > 0, (rc, rec.decision)
    ctx.map_destroy(h)
    ctx.close()

    def above():
        c2 = _native.Context(0, G.W, G.H, 16, 1400)           # kp_cap 3824: room for a map of 3801 landmarks
        try:
            Q = np.eye(4)
            Q[3, 3] = 0.0; Q[2, 3] = 50.0; Q[3, 2] = 10.0
            c2.set_Q(Q)
            c2.set_roi(*G.ROI)
            c2.upload_pair(NEW_SLOT, blank, blank, True)
            c2.plant_keypoints(NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
            hb = c2.map_create(3824)
            n = 3801
            s = map_scene(n, np.random.default_rng(47), [0, n - 1])
            c2.plant_map(hb, **s)
            kept = c2.map_download(hb)
            try:
                c2.map_track(hb, NEW_SLOT, VIEW_SLOT, G.pose_cw(), K4, Z_MIN, RATIO, ITERS, THR, SEED, 0, 10, MAXD, MAXR, SERIAL, MAX_AGE, MAX_OBS)
            except _native.VoError as e:
                assert e.code == VO_E_CAP, "status %d, want VO_E_CAP (%s)" % (e.code, e)
            else:
                raise AssertionError("a map of 3801 landmarks was not refused")
            _same_download(c2.map_download(hb), kept, "after VO_E_CAP")
            assert tuple(c2.map_view(hb, G.pose_cw(), K4, Z_MIN, NEW_SLOT, VIEW_SLOT)) == (n, n - 2)      # the unfused chain takes it
            s = map_scene(3800, np.random.default_rng(48), [0, 3799])
            c2.plant_map(hb, **s)
            r = c2.map_track(hb, NEW_SLOT, VIEW_SLOT, G.pose_cw(), K4, Z_MIN, RATIO, ITERS, THR, SEED, 0, 10, MAXD, MAXR, SERIAL, MAX_AGE, MAX_OBS)
            assert tuple(r["view"]) == (3800, 3798) and r["decision"] in (0, 2), (tuple(r["view"]), r["decision"])      # 3800 is taken
        finally:
            c2.close()
    G._guard(out, "map_above_3800", above)
    print("MAP-RESULT " + json.dumps(out))


# ---------------------------------------------------------------------------------------------- in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, env=None, timeout=240):
    key = (body, tuple(sorted((env or {}).items())))
    if key not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_map_fused as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks, **(env or {})), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("MAP-RESULT ")]
        _RESULTS[key] = (r.returncode, json.loads(lines[-1][len("MAP-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("MAP-RESULT ")))
    code, res, tail = _RESULTS[key]
    assert code == 0 and res is not None, tail
    return res


@pytest.mark.parametrize("name", ["n%d" % n for n in PAD_SIZES] + ["nothing_visible"])
def test_padded_view_is_the_view_and_row_0s_clones(name):
    res = _child("_pad_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", list(STEP_MODES))
def test_step_equals_the_unfused_chain_and_the_restatement(name):
    res = _child("_step_body()")[name]
    assert res["ok"], res["err"]
    if name == "cross_check":
        assert res["stolen"] >= 30


@pytest.mark.parametrize("name", list(DECISIONS))
def test_decisions(name):
    res = _child("_decision_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", list(FAULT_DECISIONS))
def test_decisions_only_a_fault_reaches(name):
    res = _child("_fault_body(%r)" % name, env={FAULT_DECISIONS[name][0]: "1"})[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_leave_the_map_unchanged(name):
    res = _child("_refusal_body()")[name]
    assert res["ok"], res["err"]


# ---- the odometer (the product library, in this process)
@pytest.mark.parametrize("name,kw", [("default", {}), ("cross-window", dict(cross_check=True, match_window=(24, 16)))])
def test_fused_map_odometer_equals_the_cpu_chain(oracle, name, kw):
    """C1 frames 0-7, 500 features: accept flags, skip_cause, skipped_frames, track_source and the counts of every view and update
    equal the restated fused chain (MapFusedRefOdometer on the oracle's ORB), c_T_w to 1e-9; every tracked frame is ONE map call and
    none of the unfused chain's; the unfused odometer on the same camera agrees in every decision and count, and in c_T_w to 1e-9."""
    from openvo_amd import StereoCamera, StereoOdometer, _native
    from openvo_amd.synth import Corridor
    ctx = _native.Context(0, 640, 480, 64, 500)
    try:
        c = Corridor("C1")
        cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)
        frames = c.pairs(0, 8)
        base = dict(G.BASE, **kw)
        ref = F.MapFusedRefOdometer(oracle, cam.Q, cam.valid_region_left, frames={}, **kw)
        calls = {"map_track": 0, "map_view": 0, "map_update": 0, "pnp": 0}
        real = {n: getattr(ctx, n) for n in ("map_track", "map_view", "map_update", "pnp_pair", "pnp_pair_window")}

        def counting(name, key):
            def f(*a, **k):
                calls[key] += 1
                return real[name](*a, **k)
            return f
        for n, key in (("map_track", "map_track"), ("map_view", "map_view"), ("map_update", "map_update"), ("pnp_pair", "pnp"), ("pnp_pair_window", "pnp")):
            setattr(ctx, n, counting(n, key))
        odo = StereoOdometer(cam, track="map", map_fused=True, **base)
        got = []
        for k, (L, R) in enumerate(frames):
            want = (ref.update(L, R), ref.skip_cause, ref.skipped_frames, ref.track_source)
            g = (odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.track_source)
            assert g == want, (k, g, want)
            assert {n: tuple(int(x) for x in v) for n, v in odo.map_counts.items()} == {n: tuple(int(x) for x in v) for n, v in ref.map_counts.items()}, k
            assert np.abs(odo.c_T_w - ref.c_T_w).max() <= 1e-9, (k, np.abs(odo.c_T_w - ref.c_T_w).max())
            got.append(g + (odo.c_T_w.copy(), dict(odo.map_counts)))
        assert ref.decisions == [0] * 7 and [g[3] for g in got] == [None] + ["map"] * 7
        assert calls == {"map_track": 7, "map_view": 0, "map_update": 1, "pnp": 0}, calls          # (the one update: the first frame's fold)
        lm, wm = odo.landmarks(), ref.map.download()
        for n in ("desc", "octave", "obs", "last"):
            assert np.array_equal(lm[n], wm[n]), n
        assert np.abs(lm["xyz"] - wm["xyz"]).max() <= 1e-5
        odo.release_map()
        for n in real:
            delattr(ctx, n)
        plain = StereoOdometer(cam, track="map", **base)
        for k, (L, R) in enumerate(frames):
            g = (plain.update(L, R), plain.skip_cause, plain.skipped_frames, plain.track_source)
            assert g == got[k][:4], (k, g, got[k][:4])
            assert {n: tuple(int(x) for x in v) for n, v in plain.map_counts.items()} == {n: tuple(int(x) for x in v) for n, v in got[k][5].items()}, k
            assert np.abs(plain.c_T_w - got[k][4]).max() <= 1e-9
        plain.release_map()
        print("%s: map of %d landmarks, last view %s" % (name, len(lm["xyz"]), tuple(int(x) for x in odo.map_counts["view"])))
    finally:
        ctx.close()
