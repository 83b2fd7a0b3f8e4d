"""The local-optimisation rounds of the fused PnP step (vo_pnp_pair_lo / _begin_lo / _end_lo: the LO form of k_pnp_finish in
csrc/ransac.hip; vo_track_map_lo in csrc/map.hip) on PLANTED slots and maps, against the numpy restatement tests/pnp_lo_ref.py.
The cases and their model are tests/planted_pnp_lo.py; tests/test_pnp_lo_ref.py asserts without a GPU that every case is admitted
(sequential, thread-strided and longdouble sums give the same float32 P and the same set in every round) and reaches its regime.

Every case x (rounds, steps), through pnp_pair_lo(..., want_matches=True):
    mask[:n] == S_c, mask[n:nq] == 0; lo_rounds, lo_support, refine_status, refine_steps equal the restatement's
    Rt_refined within 1e-9 of the restatement with float64 sums AND with longdouble sums (the project's bar for the refit)
    matches, n, flags, best_iter, best_count, Rt, q, t equal the plain pnp_pair's bit for bit: the RANSAC's result stays inspectable
    rounds = 1: Rt_refined is the plain entry's Rt12_refined bit for bit
    pnp_pair_begin_lo / pnp_pair_end_lo equal the synchronous call in every field; the plain pnp_pair_end ends an LO ticket too
    lo_rounds = 0 through the new entries: every output np.array_equal with the old entries', lo2 = (0, best_count)
and once: a ticket keeps its rounds while other steps (other rounds, the plain entry) run between begin and end; the refused
arguments (lo_rounds outside 0 .. 8, rounds without refine steps) are VO_E_ARG at the C ABI.

vo_track_map_lo on a planted map of 600 landmarks against (a) the unfused chain on a twin map (vo_map_view + vo_pnp_pair_lo + the
host's decisions + vo_map_update with S_c) and (b) map_fused_ref.track around the RESTATED LO step: one accepted frame with one-pixel
noise (the set changes from round to round), one frame whose winner holds fewer than 6 points (no round can run: the winner and
its own mask are what the map sees).  The counts of the update are equal, the record carries (rounds, support).

One child process per group, VO355_LIB pointing at the test-only library."""
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
import planted_pnp as PP                   # noqa: E402
import planted_pnp_lo as PLO               # noqa: E402
import pnp_lo_ref as PL                    # noqa: E402
import test_gpu_map as G                   # noqa: E402  (the map scenes' helpers: nothing of it is collected from here)
import test_gpu_map_fused as MF            # noqa: E402  (likewise)
import test_gpu_planted_pnp as T           # noqa: E402  (likewise: the context, planting, the full-length records)

pytestmark = pytest.mark.gpu

ROOT = T.ROOT
BAR_REFIT = T.BAR_REFIT                    # 1e-9
RANSAC_KEYS = ("matches", "n", "flags", "best_iter", "best_count")
VO_E_ARG = -1


# ------------------------------------------------------------------------------------------------ in the child process
def _lo_sync(ctx, c, rounds, steps):
    a, kw = T._args(c, 0, 1)
    kw.update(refine=steps, window=c.window, loop=c.loop)
    T._poison(ctx)
    return T._full(ctx, ctx.pnp_pair_lo(*a, rounds, **kw), c.nq)


def _lo_begin(ctx, c, rounds, steps, sa=0, sb=1):
    a, kw = T._args(c, sa, sb)
    kw.update(refine=steps, window=c.window, loop=c.loop)
    return ctx.pnp_pair_begin_lo(*a, rounds, **kw)


def _lo_end(ctx, c, ticket, plain=False):
    T._poison(ctx)
    return T._full(ctx, (ctx.pnp_pair_end if plain else ctx.pnp_pair_end_lo)(ticket, want_matches=True), c.nq)


def _plain(ctx, c, steps):
    a, kw = T._args(c, 0, 1)
    kw["refine"] = steps
    T._poison(ctx)
    return T._full(ctx, ctx.pnp_pair(*a, **kw), c.nq)


def _same(a, b, what, keys=T.SCALARS + ("lo_rounds", "lo_support")):
    for k in keys:
        assert a[k] == b[k], "%s: %s %s != %s" % (what, k, a[k], b[k])
    for k in ("Rt", "Rt_refined", "mask", "q", "t"):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _hold_lo(c, m, lm, r, plain, rounds, steps):
    """one LO record against the restatement and the plain entry's record -> the largest |Rt_refined - restatement|"""
    n = m["n"]
    for k in RANSAC_KEYS:
        assert r[k] == plain[k], "%s: %s != the plain entry's %s" % (k, r[k], plain[k])
    for k in ("Rt", "q", "t"):
        assert np.array_equal(r[k], plain[k]), "%s differs from the plain entry's" % k
    assert np.array_equal(plain["mask"][:n], m["mask"]), "the winner's mask is not the oracle's"
    assert (r["lo_rounds"], r["lo_support"]) == (lm["rounds"], lm["support"]), "(rounds, support) = (%d, %d), want (%d, %d)" % (
        r["lo_rounds"], r["lo_support"], lm["rounds"], lm["support"])
    assert (r["refine_status"], r["refine_steps"]) == (lm["status"], lm["steps"]), "refine2 = (%d, %d), want (%d, %d)" % (
        r["refine_status"], r["refine_steps"], lm["status"], lm["steps"])
    assert np.array_equal(r["mask"][:n], lm["mask"]), "mask differs from S_c in %d places" % int((r["mask"][:n] != lm["mask"]).sum())
    assert not r["mask"][n:].any(), "the tail of mask is not 0"
    assert int(r["mask"].sum()) == r["lo_support"]
    if lm["status"] != 0:
        assert np.array_equal(r["Rt_refined"], r["Rt"]), "no completed round: Rt_refined must be the winner"
        return 0.0
    d64, dld = float(np.abs(r["Rt_refined"] - lm["Rt"]).max()), float(np.abs(r["Rt_refined"] - lm["Rt_ld"]).max())
    assert d64 <= BAR_REFIT and dld <= BAR_REFIT, "the LO pose differs from the restatement by %.3g (float64 sums) / %.3g (longdouble sums)" % (d64, dld)
    if rounds == 1:
        assert np.array_equal(r["Rt_refined"], plain["Rt_refined"]) and plain["refine_status"] == 0, "one round is not the plain refit bit for bit"
    return max(d64, dld)


def _check_run(ctx, O, c, rounds, steps):
    m = c.model(O)
    lm = PLO.lo_model(c, O, rounds, steps)
    assert PLO.admitted(lm), "the case is not admitted: the three restatements disagree or a point sits on the threshold"
    plain = _plain(ctx, c, steps)
    r = _lo_sync(ctx, c, rounds, steps)
    print("%s R%d x %d: n %d winner %d -> rounds %d support %d status %d steps %d; want rounds %d supports %s" % (
        c.name, rounds, steps, r["n"], r["best_count"], r["lo_rounds"], r["lo_support"], r["refine_status"], r["refine_steps"], lm["rounds"],
        [int(S.sum()) for _, S in lm["trace"]]), flush=True)
    dR = _hold_lo(c, m, lm, r, plain, rounds, steps)
    print("    largest |LO pose - restatement| = %.3g" % dR, flush=True)
    _same(r, _lo_end(ctx, c, _lo_begin(ctx, c, rounds, steps)), "pnp_pair_lo and pnp_pair_begin_lo / _end_lo")
    _same(r, _lo_end(ctx, c, _lo_begin(ctx, c, rounds, steps), plain=True), "an LO ticket ended by the plain pnp_pair_end", keys=T.SCALARS)
    # no rounds through the new entries: the old entries, output for output
    z = _lo_sync(ctx, c, 0, steps)
    T._same_record(z, plain, "pnp_pair_lo(lo_rounds=0) and pnp_pair")
    assert (z["lo_rounds"], z["lo_support"]) == (0, plain["best_count"])
    z2 = _lo_end(ctx, c, _lo_begin(ctx, c, 0, steps))
    T._same_record(z2, plain, "pnp_pair_begin_lo(lo_rounds=0) / _end_lo and pnp_pair")
    assert (z2["lo_rounds"], z2["lo_support"]) == (0, plain["best_count"])
    return dict(n=r["n"], winner=r["best_count"], rounds=r["lo_rounds"], support=r["lo_support"], status=r["refine_status"], dR=dR)


def _cases_body():
    from oracle import oracle as O
    ctx = T._small_context()
    out = {}
    for c, runs in PLO.CASES:
        T._plant(ctx, c)
        for rounds, steps in runs:
            G._guard(out, "%s-R%d-s%d" % (c.name, rounds, steps), lambda: _check_run(ctx, O, c, rounds, steps))
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


def _tickets_case(ctx, O):
    """an LO ticket (3 rounds) on pair A stays what it was begun as while pair B runs 1 and 8 rounds and the plain entry, and while
    a second LO ticket with other rounds is open on the same pair"""
    a, b = PLO.case("n257"), PLO.case("n255")
    T._plant(ctx, a, 0, 1)
    T._plant(ctx, b, 2, 3)
    want3, want2 = _lo_sync(ctx, a, 3, 3), _lo_sync(ctx, a, 2, 5)
    assert not np.array_equal(want3["mask"], want2["mask"]) or not np.array_equal(want3["Rt_refined"], want2["Rt_refined"])
    t3 = _lo_begin(ctx, a, 3, 3)
    t2 = _lo_begin(ctx, a, 2, 5)
    args, kw = T._args(b, 2, 3)
    for rounds in (1, 8):
        ctx.pnp_pair_lo(*args, rounds, **dict(kw, refine=3))
    ctx.pnp_pair(*args, **dict(kw, refine=3))
    tb = ctx.pnp_pair_begin(*args, **dict(kw, refine=3))
    _same(want3, _lo_end(ctx, a, t3), "the ticket begun with 3 rounds")
    rb = T._full(ctx, ctx.pnp_pair_end_lo(tb, want_matches=True), b.nq)          # a plain ticket ended by the LO _end: lo2 = (0, best_count)
    assert (rb["lo_rounds"], rb["lo_support"]) == (0, rb["best_count"])
    _same(want2, _lo_end(ctx, a, t2), "the ticket begun with 2 rounds")
    return dict(supports=[int(want3["lo_support"]), int(want2["lo_support"])])


def _refused_case(ctx):
    import ctypes
    from openvo_amd import _native
    c = PLO.case("n7_six_grow_to_seven")
    T._plant(ctx, c)
    K4 = np.asarray(PP.K4, np.float64)
    head = [np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(12, np.float64), np.zeros(12, np.float64), np.zeros(2, np.int32)]
    lo2 = np.zeros(2, np.int32)
    L, p = ctx._lib, _native._p
    tk = ctypes.c_int(-1)
    for rounds, refine in ((-1, 3), (9, 3), (1, 0), (8, 0)):
        rc = L.vo_pnp_pair_lo(ctx._h, 0, 1, PP.RATIO, 0, p(K4), 64, PP.THR, PP.SEED, refine, *[p(a) for a in head], None, None, None, 0, rounds, p(lo2))
        assert rc == VO_E_ARG, "vo_pnp_pair_lo(lo_rounds=%d, refine_iters=%d) returned %d" % (rounds, refine, rc)
        rc = L.vo_pnp_pair_begin_lo(ctx._h, 0, 1, PP.RATIO, 0, p(K4), 64, PP.THR, PP.SEED, refine, 0, rounds, ctypes.byref(tk))
        assert rc == VO_E_ARG and tk.value == -1, "vo_pnp_pair_begin_lo(lo_rounds=%d, refine_iters=%d) returned %d" % (rounds, refine, rc)
        for call in (ctx.pnp_pair_lo, ctx.pnp_pair_begin_lo):
            with pytest.raises(ValueError):
                call(0, 1, PP.RATIO, PP.K4, rounds, refine=refine)
    rc = L.vo_pnp_pair_lo(ctx._h, 0, 1, PP.RATIO, 0, p(K4), 64, PP.THR, PP.SEED, 3, *[p(a) for a in head], None, None, None, 0, 2, None)
    assert rc == VO_E_ARG, "vo_pnp_pair_lo without lo2 returned %d" % rc
    r = ctx.pnp_pair_lo(0, 1, PP.RATIO, PP.K4, 0, iters=64, refine=0)                # no rounds and no refit is a plain call
    assert (r["lo_rounds"], r["lo_support"], r["refine_status"]) == (0, r["best_count"], 1)
    return {}


def _tickets_body():
    from oracle import oracle as O
    ctx = T._small_context()
    out = {}
    G._guard(out, "tickets_keep_their_rounds", lambda: _tickets_case(ctx, O))
    G._guard(out, "refused_arguments", lambda: _refused_case(ctx))
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


# ---- vo_track_map_lo
MAP_N, MAP_ROUNDS, MAP_STEPS = 600, 3, 3
MAP_CASES = {      # name: (matches wanted, pixel noise, share of the matches at their projection, min_matches, scene seed)
    "accepted_3_rounds": (300, 1.0, 0.7, 10, 1),
    "no_round_can_run": (9, 0.3, 0.56, 4, 4),
}                  # (the scene seeds: the first that is admitted -- seed 0 of the first case has a point 6e-5 from the threshold --
                   #  and reaches the regime; tests/test_pnp_lo_ref.py asserts both for the seeds chosen)


def map_case(name):
    """-> (scene, frame, view of the restated map, pose): deterministic, so that the CPU test can hold the case to its regime"""
    M_want, noise, share, _, seed = MAP_CASES[name]
    rng = np.random.default_rng([37, sorted(MAP_CASES).index(name), seed])
    inv = MF.pad_invisible(MAP_N, rng)
    scene = MF.map_scene(MAP_N, rng, inv)
    pose = G.pose_cw()
    probe = M.MapRef(MAP_N, G.KP_CAP)
    probe.plant(scene["xyz"], scene["desc"], scene["rdesc"], scene["octave"], scene["obs"], scene["last"])
    view = probe.view(pose, G.K4, G.Z_MIN, G.ORG, G.CROP)
    f = MF.new_frame(view, rng, M_want, noise=noise, at_projection=share)
    return scene, f, view, pose


def map_lo_model(O, view, f):
    """G.pnp_model + the restated rounds three ways -> (m, lo dict as planted_pnp_lo.lo_model's)"""
    m = G.pnp_model(O, view, f)
    X = np.ascontiguousarray(view["xyz"][m["q"]])
    uv = np.ascontiguousarray(f["xy"][m["t"]] + np.float32(G.ORG)).astype(np.float32).reshape(-1, 2)
    a = (m["Rt"], m["mask"], X, uv, G.K4, G.THR, MAP_STEPS, MAP_ROUNDS)
    t0, t1, t2 = [], [], []
    Rt, S, status, nsteps, done = PL.lo(*a, trace=t0)
    _, _, st_s, _, done_s = PL.lo(*a, order=PP.strided_order, trace=t1)
    Rl, _, st_l, _, done_l = PL.lo(*a, dtype=np.longdouble, trace=t2)
    margin = min([PL.select_margin(Pm, X, uv, G.THR) for Pm, _ in t0] or [float("inf")])
    return m, dict(Rt=Rt, mask=S, status=status, steps=nsteps, rounds=done, support=int(S.sum()), trace=t0, trace_strided=t1, trace_ld=t2, Rt_ld=Rl,
                   others=((st_s, done_s), (st_l, done_l)), margin=margin)


def _map_case(ctx, O, name):
    scene, f, view, pose = map_case(name)
    mm = MAP_CASES[name][3]
    m, lm = map_lo_model(O, view, f)
    assert PLO.admitted(lm), "the case is not admitted"
    h, h2 = ctx.map_create(MAP_N + 400), ctx.map_create(MAP_N + 400)
    try:
        ref = M.MapRef(MAP_N + 400, G.KP_CAP)
        MF._plant(ctx, (h, h2), ref, scene)
        ctx.plant_keypoints(MF.NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        # the unfused chain on the twin, composed here: the LO pose for the gates, S_c for the update
        c2 = ctx.map_view(h2, pose, G.K4, G.Z_MIN, MF.NEW_SLOT, MF.VIEW2)
        vis = int(c2[1])
        u = ctx.pnp_pair_lo(MF.VIEW2, MF.NEW_SLOT, G.RATIO, G.K4, MAP_ROUNDS, G.ITERS, G.THR, G.SEED, MAP_STEPS, True)
        dec, Tm = MF._host_decision(u, vis, min_matches=mm)
        assert dec == 0, "the unfused chain does not accept the planted frame: decision %d" % dec
        assert (u["lo_rounds"], u["lo_support"], u["refine_status"]) == (lm["rounds"], lm["support"], lm["status"])
        assert np.array_equal(u["mask"], lm["mask"]) and np.array_equal(u["q"], m["q"]) and np.array_equal(u["t"], m["t"])
        cw_host = np.vstack([Tm, [0, 0, 0, 1]]) @ np.vstack([pose, [0, 0, 0, 1]])
        c6 = ctx.map_update(h2, MF.NEW_SLOT, np.linalg.inv(cw_host), MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS, u["q"], u["t"], u["mask"])
        # the fused step
        r = ctx.track_map_lo(h, MF.NEW_SLOT, MF.VIEW_SLOT, pose, G.K4, G.Z_MIN, G.RATIO, G.ITERS, G.THR, G.SEED, MAP_STEPS, mm, MF.MAXD, MF.MAXR,
                             MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS, MAP_ROUNDS)
        assert r["decision"] == 0 and tuple(r["view"]) == tuple(c2) and r["update_flags"] == 0, (r["decision"], tuple(r["view"]), tuple(c2))
        for k in T.SCALARS + ("lo_rounds", "lo_support"):
            assert r[k] == u[k], "%s: fused %d, unfused %d" % (k, r[k], u[k])
        for k in ("q", "t", "mask", "Rt", "Rt_refined"):
            assert np.array_equal(r[k], u[k]), "%s differs from the unfused step's" % k
        assert tuple(r["update"]) == tuple(c6), "counts6 %s, unfused %s" % (tuple(r["update"]), tuple(c6))
        assert np.abs(np.vstack([r["c_T_w"], [0, 0, 0, 1]]) - cw_host).max() <= 1e-12
        got, twin = ctx.map_download(h), ctx.map_download(h2)
        for k in ("desc", "octave", "obs", "last"):
            assert np.array_equal(got[k], twin[k]), "%s of the map differs from the unfused chain's" % k
        # the restatement around the RESTATED rounds: nothing of the step's own record goes in
        lo_rec = dict(matches=m["M"], flags=0, n=m["n"], best_count=m["best_count"], Rt=m["Rt"], Rt_refined=lm["Rt"], refine_status=lm["status"],
                      q=m["q"], t=m["t"], mask=lm["mask"])
        want = F.track(ref, f, pose, G.K4, G.Z_MIN, G.ORG, G.CROP, lambda v, fr: lo_rec, mm, MF.MAXD, MF.MAXR, MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS)
        assert want["decision"] == 0 and tuple(want["update"]) == tuple(r["update"]), "counts6 %s, the restatement's %s" % (tuple(r["update"]), tuple(want["update"]))
        if lm["status"] == 0:
            d = float(np.abs(r["Rt_refined"] - lm["Rt"]).max())
            assert d <= BAR_REFIT, "the LO pose differs from the restatement by %.3g" % d
        else:
            assert np.array_equal(r["mask"], m["mask"]) and r["lo_support"] == m["best_count"] < 6
        dcw = float(np.abs(want["c_T_w"] - r["c_T_w"]).max())
        assert dcw <= BAR_REFIT, "c_T_w differs from the restatement's by %.3g" % dcw
        wm = ref.download()
        for k in ("desc", "octave", "obs", "last"):
            assert np.array_equal(got[k], wm[k]), "%s of the map differs from the restatement's" % k
        fin = np.isfinite(wm["xyz"])
        dx = float(np.abs(got["xyz"][fin].astype(np.float64) - wm["xyz"][fin].astype(np.float64)).max())
        assert dx <= 1e-5, "xyz is %.3g from the restatement's" % dx        # (a pose within 1e-9 moves a float32 point of |X| < 30 m by ulps)
        fig = dict(vis=vis, M=r["matches"], n=r["n"], winner=r["best_count"], rounds=r["lo_rounds"], support=r["lo_support"],
                   counts6=[int(x) for x in c6], supports=[int(S.sum()) for _, S in lm["trace"]])
        print("%s: %s" % (name, fig), flush=True)
        return fig
    finally:
        ctx.map_destroy(h)
        ctx.map_destroy(h2)


def _map_body():
    from oracle import oracle as O
    ctx = G._context()
    out = {}
    for name in MAP_CASES:
        G._guard(out, name, lambda: _map_case(ctx, O, name))
    # lo_rounds == 0 IS vo_track_map: the record's two words stay 0
    scene, f, view, pose = map_case("accepted_3_rounds")

    def zero():
        recs = []
        for call in ("lo", "plain"):
            h = ctx.map_create(MAP_N + 400)
            try:
                MF._plant(ctx, (h,), None, scene)
                ctx.plant_keypoints(MF.NEW_SLOT, f["xy"], f["desc"], f["xyz"], f["rdesc"])
                a = (h, MF.NEW_SLOT, MF.VIEW_SLOT, pose, G.K4, G.Z_MIN, G.RATIO, G.ITERS, G.THR, G.SEED, 3, 10, MF.MAXD, MF.MAXR, MF.SERIAL, MF.MAX_AGE, MF.MAX_OBS)
                recs.append((ctx.track_map_lo(*a, 0) if call == "lo" else ctx.map_track(*a), ctx.map_download(h)))
            finally:
                ctx.map_destroy(h)
        (a, ma), (b, mb) = recs
        assert (a["lo_rounds"], a["lo_support"]) == (0, 0) and a["decision"] == 0
        for k in b:
            assert np.array_equal(a[k], b[k]), "track_map_lo(lo_rounds=0) and map_track differ in %s" % k
        MF._same_download(ma, mb, "track_map_lo(lo_rounds=0) and map_track")
    G._guard(out, "zero_rounds_is_vo_track_map", zero)
    ctx.close()
    print("PLANTED-RESULT " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ in the test process
_RESULTS = {}
_STOPPED = []          # a child that was killed by a signal or ran into its time limit: nothing more is started on the GPU


def _child(body, timeout=240):
    if body not in _RESULTS:
        assert not _STOPPED, "not started: the child %s ended abnormally before" % _STOPPED[0]
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        try:
            r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_planted_pnp_lo as t; t.%s" % body], cwd=ROOT,
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


@pytest.mark.parametrize("name,rounds,steps", PLO.ALL, ids=["%s-R%d-s%d" % a for a in PLO.ALL])
def test_planted_lo_rounds(name, rounds, steps):
    res = _child("_cases_body()")["%s-R%d-s%d" % (name, rounds, steps)]
    assert res["ok"], res["err"]
    print("%s R%d x %d: n %d, winner %d -> %d rounds, support %d, status %d, largest |LO pose - restatement| = %.3g" % (
        name, rounds, steps, res["n"], res["winner"], res["rounds"], res["support"], res["status"], res["dR"]))


@pytest.mark.parametrize("name", ["tickets_keep_their_rounds", "refused_arguments"])
def test_tickets_and_arguments(name):
    res = _child("_tickets_body()")[name]
    assert res["ok"], res["err"]


@pytest.mark.parametrize("name", list(MAP_CASES) + ["zero_rounds_is_vo_track_map"])
def test_track_map_lo(name):
    res = _child("_map_body()")[name]
    assert res["ok"], res["err"]
    if name == "no_round_can_run":
        assert res["rounds"] == 0 and res["support"] == res["winner"] < 6
    elif name == "accepted_3_rounds":
        assert res["rounds"] == 3 and len(set(res["supports"] + [res["winner"]])) > 1
