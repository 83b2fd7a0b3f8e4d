"""Every camera-consuming kernel behind the fused steps on a GENERIC camera (tests/camera_cases.py): fx != fy, cx != cy, neither at the
image centre, K4's principal point not Q's, Q[3][3] != 0 -- so that a kernel which reads fx for fy, cx for cy, the principal point from
Q instead of K4, or Q[3][3] from another cell no longer computes what its reference computes.  tests/test_camera_axes_ref.py asserts
on the CPU that every case reaches its regime and that each such slip moves the reference by at least 1000 x the bar it is held to here.

    recover_pose        planted_mono's builders under K_640: one vote scene per winner 0 .. 3 and a four-way tie (every candidate voted
                        on), the parallax gate with inliers on both sides, shared depths behind indices with scale_rel, n = 1025 across
                        the 1024-thread stride; held to mono_pose_ref.recover_pose exactly as test_gpu_planted_mono._check does
    mono_pose_pair      planted_mono's "eight" frames through the fused finish under K_640, compared as test_gpu_planted_mono's fused case
    pnp_pair, _window   planted_pnp cases under K_640 (M = 65, M = 300, 0.3 px noise, three refit steps; one through the windowed matcher)
    pnp_pair_lo         held by test_gpu_planted_pnp._check_case / test_gpu_planted_pnp_lo._check_run: the oracle's RANSAC exactly, Rt
                        within 1e-10, the refit and the LO pose within 1e-9 of the float64 and the longdouble restatement
    klt_pnp_pair        test_gpu_klt_pnp's sparse n = 65 pair with three refit steps, its cloud planted under the generic 160 x 120
                        camera: the composed chain and the planted route, bit for bit
    map_view            a map of 197 landmarks under K_704: inside, inside and outside each edge of the window, before and beyond
    track_map           z_min, behind the camera; the view bit for bit against map_ref.view, one fused step against map_fused_ref.track
                        around the RESTATED PnP (oracle RANSAC + float64 refit): integers exact, Rt 1e-10, Rt_refined and c_T_w 1e-9
    direct_align        the generic_* members of direct_cases.CASES run through tests/test_gpu_direct.py's own matrix
    reproject_to_3d     a Q with all 16 entries non-zero, three shapes up to 80 x 60 with zero and negative disparities: bit for bit
    points3d_at         against the oracle (which the CPU module holds to float64 Q v / (Q v)[3])

The calls that take arrays run in this process; the planted ones in ONE child process on the test-only library.  The module's last
test asserts that every entry point above was met."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as CC                  # noqa: E402
import direct_cases as DC                  # noqa: E402
import map_fused_ref as F                  # noqa: E402
import map_ref as M                        # noqa: E402
import planted as P                        # noqa: E402
import planted_mono as PM                  # noqa: E402
import pnp_refine_ref as PR                # noqa: E402
import test_gpu_klt_pnp as KT              # noqa: E402  (helpers only: nothing of these modules is collected from here)
import test_gpu_map as G                   # noqa: E402
import test_gpu_map_fused as MF            # noqa: E402
import test_gpu_planted_dense as DN         # noqa: E402
import test_gpu_planted_mono as TM         # noqa: E402
import test_gpu_planted_pnp as T           # noqa: E402
import test_gpu_planted_pnp_lo as LO       # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"recover_pose", "mono_pose_pair", "pnp_pair", "pnp_pair_window", "pnp_pair_lo", "klt_pnp_pair", "map_view", "track_map",
                "direct_align", "reproject_to_3d", "points3d_at"}
SEEN = set()
BAR_RT, BAR_REFIT = T.BAR_RT, T.BAR_REFIT  # 1e-10, 1e-9


# ---- the map case (no GPU in here: tests/test_camera_axes_ref.py holds it to its regime) --------------------------------------------------
MAP_REFINE, MAP_MIN_MATCHES, MAP_M = 3, 10, 100
_map_inputs = []


def map_inputs():
    """-> (scene, kind per landmark, pose, frame): planted under K_704, built once"""
    if not _map_inputs:
        pose = G.pose_cw()
        scene, kind = CC.map_scene(pose, CC.K_704, G.Z_MIN, G.ORG, G.CROP)
        probe = M.MapRef(scene["capacity"], G.KP_CAP)
        MF._plant(None, (), probe, scene)
        view = probe.view(pose, CC.K_704, G.Z_MIN, G.ORG, G.CROP)
        frame = CC.map_frame(view, CC.K_704, G.ORG, G.CROP, P._motion(), np.random.default_rng(93), MAP_M)
        _map_inputs.append((scene, kind, pose, frame))
    return _map_inputs[0]


def restated_pnp(O, K4):
    """the PnP function map_fused_ref.track is built around: numpy matches, the finite filter, the oracle's RANSAC, the float64 refit"""
    def pnp(view, frame):
        vis = view["vis"]
        q, t = P.matches(view["desc"][:vis], frame["desc"], G.RATIO)
        X = view["xyz"][q]
        ok = np.isfinite(X).all(1)
        M_, q, t, X = len(ok), q[ok], t[ok], np.ascontiguousarray(X[ok])
        uv = np.ascontiguousarray(frame["xy"][t] + np.float32(G.ORG)).astype(np.float32).reshape(-1, 2)
        r = O.ransac_pnp(X, uv, K4, G.ITERS, G.THR, G.SEED)
        Rt = np.array(r["Rt"]).reshape(3, 4)
        Rt64, status, steps = PR.refine(Rt, X, uv, K4, r["mask"], MAP_REFINE)
        return dict(matches=M_, flags=0, n=len(q), best_iter=r["best_iter"], best_count=r["best_count"], Rt=Rt, Rt_refined=Rt64, refine_status=status,
                    refine_steps=steps, q=q, t=t, mask=r["mask"].copy())
    return pnp


def map_model(O, K4):
    """the view and one fused step of the restated map under the camera K4 -> (view, record, the map after the step)"""
    scene, _, pose, frame = map_inputs()
    ref = M.MapRef(scene["capacity"], G.KP_CAP)
    MF._plant(None, (), ref, scene)
    view = ref.view(pose, K4, G.Z_MIN, G.ORG, G.CROP)
    rec = F.track(ref, frame, pose, K4, G.Z_MIN, G.ORG, G.CROP, restated_pnp(O, K4), MAP_MIN_MATCHES, MF.MAXD, MF.MAXR, MF.SERIAL, MF.MAX_AGE,
                  MF.MAX_OBS)
    return view, rec, ref


# ---- the arrays of the dense lookups ---------------------------------------------------------------------------------------------------------
def lookup_positions(w, h):
    """crop pixels of points3d_at: random sub-pixel positions, integer positions, the last column and the last row (taps that do not exist)"""
    rng = np.random.default_rng([95, w, h])
    xy = np.stack([rng.uniform(0, w - 1, 60), rng.uniform(0, h - 1, 60)], 1)
    edge = [[w - 1, 0.5], [w - 1, h - 1], [0.25, h - 1], [0, 0], [w - 2, h - 2], [3, 2]]
    return np.concatenate([xy, np.array(edge, np.float64)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ in the child process
def _pnp_part(O, out):
    ctx = T._small_context()
    cases = CC.pnp_cases()
    for key in ("M65", "M300", "window"):
        G._guard(out, "pnp_" + key, lambda: T._check_case(ctx, O, cases[key]))
    c = cases["lo"]
    T._plant(ctx, c)
    G._guard(out, "pnp_lo", lambda: LO._check_run(ctx, O, c, *CC.LO_RUN))
    ctx.close()


def _klt_part(out):
    import klt_cases as C
    ctx = KT._context()
    a, b = C.smooth_pair(KT.W, KT.H)
    G._guard(out, "klt_pnp", lambda: KT._check_case(ctx, a, b, CC.KLT_CASE))
    ctx.close()


def _map_step(ctx, O):
    K4 = CC.K_704
    scene, _, pose, f = map_inputs()
    view, want, ref_after = map_model(O, K4)
    h = ctx.map_create(scene["capacity"])
    try:
        MF._plant(ctx, (h,), None, scene)
        ctx.plant_keypoints(MF.NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        r = ctx.map_track(h, MF.NEW_SLOT, MF.VIEW_SLOT, pose, K4, G.Z_MIN, G.RATIO, G.ITERS, G.THR, G.SEED, MAP_REFINE, MAP_MIN_MATCHES, MF.MAXD, MF.MAXR,
                          MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS)
        assert r["decision"] == want["decision"] == 0, "decision %d, the restatement's %d" % (r["decision"], want["decision"])
        assert tuple(r["view"]) == tuple(want["view"]) and r["update_flags"] == 0, (tuple(r["view"]), tuple(want["view"]))
        for k in ("matches", "n", "flags", "best_iter", "best_count", "refine_status", "refine_steps"):
            assert r[k] == want[k], "%s: %d, the restatement's %d" % (k, r[k], want[k])
        for k in ("q", "t", "mask"):
            assert np.array_equal(r[k], want[k]), "%s differs from the restatement's" % k
        d_rt, d_ref = float(np.abs(r["Rt"] - want["Rt"]).max()), float(np.abs(r["Rt_refined"] - want["Rt_refined"]).max())
        d_cw = float(np.abs(r["c_T_w"] - want["c_T_w"]).max())
        print("track_map: vis %d, M %d, n %d, best %d @ %d, refit %d / %d | Rt %.2e, Rt_refined %.2e, c_T_w %.2e from the restatement" % (
            r["view"][1], r["matches"], r["n"], r["best_count"], r["best_iter"], r["refine_status"], r["refine_steps"], d_rt, d_ref, d_cw), flush=True)
        assert r["refine_status"] == 0 and d_rt <= BAR_RT and d_ref <= BAR_REFIT and d_cw <= BAR_REFIT
        assert tuple(r["update"]) == tuple(want["update"]), "counts6 %s, the restatement's %s" % (tuple(r["update"]), tuple(want["update"]))
        got, wm = ctx.map_download(h), ref_after.download()
        for k in ("desc", "octave", "obs", "last"):
            assert np.array_equal(got[k], wm[k]), "%s of the map differs from the restatement's" % k
        fin = np.isfinite(wm["xyz"])
        dx = float(np.abs(got["xyz"][fin].astype(np.float64) - wm["xyz"][fin].astype(np.float64)).max())
        assert dx <= 1e-5, "xyz is %.3g from the restatement's" % dx          # (a pose within 1e-9 moves a float32 point of |X| < 30 m by ulps)
        # the restatement fed the step's own PnP record: the composed pose and its inverse bit for bit, the map bit for bit
        ref2 = M.MapRef(scene["capacity"], G.KP_CAP)
        MF._plant(ctx, (), ref2, scene)
        own = F.track(ref2, f, pose, K4, G.Z_MIN, G.ORG, G.CROP, lambda v, fr: {k: r[k] for k in ("matches", "flags", "n", "best_count", "Rt", "Rt_refined",
                                                                                                   "refine_status", "q", "t", "mask")},
                      MAP_MIN_MATCHES, MF.MAXD, MF.MAXR, MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS)
        assert np.array_equal(own["c_T_w"], r["c_T_w"]) and np.array_equal(own["w_T_c"], r["w_T_c"]), "c_T_w / w_T_c are not the restatement's bit for bit"
        G._same_map(ctx, h, ref2)
        G._same_view(ctx, ctx.map_view(h, pose, K4, G.Z_MIN, MF.NEW_SLOT, MF.VIEW_SLOT), ref2.view(pose, K4, G.Z_MIN, G.ORG, G.CROP), slot=MF.VIEW_SLOT)
        return dict(dRt=d_rt, dRefit=d_ref, dcw=d_cw, vis=int(r["view"][1]), best_count=int(r["best_count"]))
    finally:
        ctx.map_destroy(h)


def _map_part(O, out):
    ctx = G._context()
    scene, _, pose, _ = map_inputs()
    G._guard(out, "map_view", lambda: G._view_case(ctx, O, "generic_view", scene, pose, CC.K_704, pnp=False))
    G._guard(out, "track_map", lambda: _map_step(ctx, O))
    ctx.close()


def _points_part(O, out):
    from openvo_amd import _native
    ctx = _native.Context(0, 96, 64, 16, 1024)          # (a context is at least 64 x 64: the planted fields are smaller)

    def check():
        n = 0
        for w, h in CC.REPROJECT_SHAPES:
            Q = CC.full_Q(w, h)
            disp16 = np.rint(16.0 * CC.disparity(w, h)).astype(np.int16)
            ctx.set_Q(Q)
            ctx.plant_dense(0, disp16, *DN._one_kp())
            xy = lookup_positions(w, h)
            got, st = ctx.points3d_at(0, xy)
            want, wst = O.points3d_at(disp16, Q, DN._roi4(None), xy)
            DN._same_lookup(got, st, want, wst, ("points3d_at", w, h))
            assert (wst == 0).sum() >= 60
            DN._same_image(ctx.download_xyz(0, (h, w)), O.reproject_to_3d(disp16.astype(np.float32) / np.float32(16.0), Q), ("xyz", w, h))
            n += len(xy)
        return dict(n=n)
    G._guard(out, "points3d_at", check)
    ctx.close()


def _planted_body():
    from oracle import oracle as O
    O.build_oracle()
    out = {}
    _pnp_part(O, out)
    _klt_part(out)
    _map_part(O, out)
    _points_part(O, out)
    print("AXES-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_camera_axes as t; t.%s" % body], cwd=ROOT,
                               env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            _STOPPED.append(body)
            raise
        if r.returncode < 0 or r.returncode > 128:
            _STOPPED.append(body)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("AXES-RESULT ")]
        _RESULTS[body] = (r.returncode, json.loads(lines[-1][len("AXES-RESULT "):]) if lines else None, r.stdout[-6000:] + r.stderr[-4000:])
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("AXES-RESULT ")))
    code, res, tail = _RESULTS[body]
    assert code == 0 and res is not None, tail
    return res


PLANTED = {"pnp_M65": "pnp_pair", "pnp_M300": "pnp_pair", "pnp_window": "pnp_pair_window", "pnp_lo": "pnp_pair_lo", "klt_pnp": "klt_pnp_pair",
           "map_view": "map_view", "track_map": "track_map", "points3d_at": "points3d_at"}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_step_on_the_generic_camera(name):
    res = _child("_planted_body()")[name]
    assert res["ok"], res["err"]
    print("%s: %s" % (name, {k: v for k, v in res.items() if k != "ok"}))
    SEEN.add(PLANTED[name])


@pytest.fixture(scope="module")
def ctx():
    from openvo_amd import _native
    c = _native.Context(0, 640, 480, 16, 2000)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    return CC.mono_scenes()


@pytest.mark.parametrize("name", list(CC.MONO_VOTES) + ["gate", "shared_depth", "n1025"])
def test_recover_pose_on_the_generic_camera(ctx, scenes, name):
    s = scenes[name]
    E, p1, p2, K4, mask, q, t, na, nb, depth_a, gate = CC.mono_args(s, CC.K_640)
    got, r = TM._check(ctx, E, p1, p2, mask, q, t, na, nb, depth_a, gate, K4=K4)
    rel = [float(np.max(np.abs(got[k] - r[k]) / np.where(r[k] != 0, np.abs(r[k]), 1.0))) for k in ("z1", "z2", "depth_b")]
    print("%s: n %d, votes %s, winner %d, n_depth %d, n_shared %d, scale_rel %.17g | z1 %.1e, z2 %.1e, depth_b %.1e relative, R %.1e, t %.1e" % (
        name, len(p1), got["votes4"].tolist(), got["winner"], got["n_depth"], got["n_shared"], got["scale_rel"], rel[0], rel[1], rel[2],
        float(np.abs(got["R"] - r["R"]).max()), float(np.abs(got["t"] - r["t"]).max())))
    assert got["flags"] == 0
    if "counts4" in s:
        assert list(got["votes4"]) == list(s["counts4"]) and all(got["votes4"])
    if name.startswith("winner"):
        assert got["winner"] == int(name[-1])
    if name == "gate":
        assert 4 < got["n_depth"] < 20 and np.array_equal(got["depth_b"] != 0, s["sin2"] >= PM.GATE)
    if name == "shared_depth":
        assert got["n_depth"] == 50 and 30 <= got["n_shared"] < 50 and got["scale_rel"] > 0 and len(got["depth_b"]) == nb
    SEEN.add("recover_pose")


def test_mono_pose_pair_on_the_generic_camera(ctx):
    seed, M_want = PM.FINISH_SEEDS["eight"]
    K4 = list(CC.K_640)
    xy = []
    for slot, frame in zip((20, 21), PM.finish_frames(seed)):
        ctx.upload_mono(slot, frame)
        assert ctx.orb_slot_count(slot, 2000, 0) >= 3
        xy.append(ctx.download_keypoints_xy(slot))
    na, nb = len(xy[0]), len(xy[1])
    args = (PM.FINISH_RATIO, K4) + CC.MONO_PAIR_ARGS
    got = ctx.mono_pose_pair(20, 21, *args, 8, False, prev_serial=0, min_parallax_sin2=0.0)
    print("mono_pose_pair: %d keypoints, %d matches, best_count %d, flags %d, votes %s, winner %d, n_depth %d" % (
        na, got["matches"], got["best_count"], got["flags"], got["votes4"].tolist(), got["winner"], got["n_depth"]))
    assert got["matches"] == M_want and got["best_count"] >= 1 and not (got["flags"] & 1)      # (as the CPU chain: a pose was recovered)
    depth, serial = ctx.download_mono_depth(21)
    assert serial == got["serial"] != 0 and len(depth) == nb
    comp = ctx.mono_pair(20, 21, *args, want_matches=True, solver=8)
    assert (comp["matches"], comp["best_iter"], comp["best_count"]) == (got["matches"], got["best_iter"], got["best_count"])
    assert np.array_equal(got["E"], comp["E"]) and len(comp["q"]) == M_want
    p1, p2 = xy[0][comp["q"]], xy[1][comp["t"]]
    rp, _ = TM._check(ctx, comp["E"], p1, p2, comp["mask"], comp["q"], comp["t"], na, nb, None, 0.0, K4=K4)
    for k in ("winner", "n_depth", "n_shared", "flags", "scale_rel"):
        assert got[k] == rp[k], (k, got[k], rp[k])
    for k in ("votes4", "R", "t"):
        assert np.array_equal(got[k], rp[k]), k
    assert np.array_equal(depth, rp["depth_b"])
    SEEN.add("mono_pose_pair")


@pytest.mark.parametrize("w,h", CC.REPROJECT_SHAPES)
def test_reproject_to_3d_with_a_full_Q(ctx, oracle, w, h):
    Q, disp = CC.full_Q(w, h), CC.disparity(w, h)
    assert np.count_nonzero(Q) == 16 and (disp == 0).any() and (disp < 0).any()
    got, want = ctx.reproject_to_3d(disp, Q), oracle.reproject_to_3d(disp, Q)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d values differ from the oracle in their bits" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    SEEN.add("reproject_to_3d")


def test_every_entry_point_met_the_generic_camera():
    generic = [c.name for c in DC.CASES if c.opt.get("rig") == "generic"]
    assert len(generic) >= 5                       # (tests/test_gpu_direct.py runs every member of CASES through its matrix)
    SEEN.add("direct_align")
    assert SEEN == ENTRY_POINTS, sorted(ENTRY_POINTS - SEEN)
