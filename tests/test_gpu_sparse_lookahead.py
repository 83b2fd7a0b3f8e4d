"""Sparse stereo begun ahead: the vo_prefetch_*_sparse entries (the whole chain on a look-ahead engine, collected by vo_sparse_stereo
from the slot's own record) against the synchronous call and the numpy restatement, the pose steps on collected slots, and
StereoCamera.submit_sparse / StereoOdometer.run() in sparse mode against the update() chain.  Context(0, 640, 480, 64, 500), C1
corridor frames; every synchronous reference is computed once per module."""
import numpy as np
import pytest

import sparse_stereo_ref as S
from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.stereo_camera import _RESERVED
from openvo_amd.synth import Corridor

pytestmark = pytest.mark.gpu

VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
NF = 500
PARAMS = (4, 100, 2.0, 75)
OTHER = (4, 60, 1.0, 60)
RATIO, ITERS, THR, SEED = 0.8, 256, 1.5, 4321
KP = ("xy", "size", "angle", "response", "octave", "desc")


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 640, 480, 64, 500)
    yield c
    c.close()


def _camera(ctx, name):
    c = Corridor(name)
    return c, StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _slot_arrays(ctx, slot):
    got = ctx.download_keypoints(slot)
    got["xyz"], got["disp"] = ctx.download_keypoint_depth(slot)
    return got


def _same(got, want, c3=None, want_c3=None):
    if c3 is not None:
        assert np.array_equal(c3, want_c3), (c3, want_c3)
    for k in KP:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["disp"]), _bits(want["disp"])) and np.array_equal(_bits(got["xyz"]), _bits(want["xyz"]))


@pytest.fixture(scope="module")
def rig(ctx):
    """C1 frames 0 - 7; frames 0 - 3 computed synchronously in slots 24 - 27 (the reference every slot-level test shares), frame 0
    once more with the OTHER request, and the restatement of each on the library's own ORB of the two crops"""
    c, cam = _camera(ctx, "C1")
    frames = c.pairs(0, 8)
    sync, restated = [], []
    for k in range(4):
        ctx.upload_pair(24 + k, *frames[k], True)
        c3 = ctx.sparse_stereo(24 + k, NF, *PARAMS)
        sync.append(dict(_slot_arrays(ctx, 24 + k), c3=c3))
        restated.append(S.sparse_frame(None, *frames[k], cam.Q, cam.valid_region_left, NF, *PARAMS, orb=lambda img: ctx.orb_host(img, None, NF)))
    ctx.upload_pair(23, *frames[0], True)
    c3 = ctx.sparse_stereo(23, NF, *OTHER)
    other = dict(_slot_arrays(ctx, 23), c3=c3)
    return dict(c=c, cam=cam, frames=frames, sync=sync, restated=restated, other=other)


# ---- slot level --------------------------------------------------------------------------------------------------------------------
def test_four_pairs_on_two_engines_collected_in_reverse(ctx, rig):
    """Two pairs per engine with no collection in between: each engine's scratch (keypoint sets, count words, match / disp / xyz) is
    reused by its second pair before the host has read anything -- what the host reads lies in the slots."""
    cam, frames = rig["cam"], rig["frames"]
    engines = ctx.set_engines(0)
    try:
        assert ctx.set_engines(2) == 2
        cam.stage_pairs(frames[:4])
        assert ctx.lookahead_depth() == 0
        for k in range(4):
            ctx.prefetch_staged_pair_sparse(k, k, True, NF, *PARAMS)
        assert ctx.lookahead_depth() == 4
        for k in (3, 2, 1, 0):
            c3 = ctx.sparse_stereo(k, NF, *PARAMS)
            got = _slot_arrays(ctx, k)
            _same(got, rig["sync"][k], c3, rig["sync"][k]["c3"])
            _same(got, rig["restated"][k], c3, rig["restated"][k]["counts3"])
            assert np.array_equal(ctx.sparse_stereo(k, NF, *PARAMS), c3)       # collected: the counts again, nothing recomputed
            assert ctx.lookahead_depth() == k
            assert c3[2] >= 200
    finally:
        ctx.set_engines(engines)


def test_collecting_with_another_request_recomputes(ctx, rig):
    cam, frames = rig["cam"], rig["frames"]
    cam.stage_pairs(frames[:4])
    ctx.prefetch_staged_pair_sparse(5, 0, True, NF, *PARAMS)
    c3 = ctx.sparse_stereo(5, NF, *OTHER)
    _same(_slot_arrays(ctx, 5), rig["other"], c3, rig["other"]["c3"])
    assert ctx.lookahead_depth() == 0
    assert not np.array_equal(c3, rig["sync"][0]["c3"])


def test_a_new_q_voids_what_was_begun_ahead_and_synchronous_calls_always_recompute(ctx, rig):
    """Only a slot begun ahead and collected returns its counts again; vo_set_Q (and vo_set_roi) void that and a pending chain: the
    next call computes with the Q in force.  A synchronous result is never reused."""
    cam, frames = rig["cam"], rig["frames"]
    Q2 = np.array(cam.Q, np.float64)
    Q2[2, 3] *= 1.25
    cam.stage_pairs(frames[:1])
    ctx.prefetch_staged_pair_sparse(12, 0, True, NF, *PARAMS)
    ctx.prefetch_staged_pair_sparse(13, 0, True, NF, *PARAMS)
    ctx.sparse_stereo(12, NF, *PARAMS)                                          # 12: collected, 13: pending
    try:
        ctx.set_Q(Q2)
        ctx.upload_pair(22, *frames[0], True)
        c3 = ctx.sparse_stereo(22, NF, *PARAMS)
        want2 = dict(_slot_arrays(ctx, 22), c3=c3)
        assert not np.array_equal(_bits(want2["xyz"]), _bits(rig["sync"][0]["xyz"]))
        for s in (12, 13):
            c3 = ctx.sparse_stereo(s, NF, *PARAMS)
            _same(_slot_arrays(ctx, s), want2, c3, want2["c3"])
        assert ctx.lookahead_depth() == 0
    finally:
        ctx.set_Q(cam.Q)
    c3 = ctx.sparse_stereo(22, NF, *PARAMS)                                     # the same request on a synchronously filled slot: computed again
    _same(_slot_arrays(ctx, 22), rig["sync"][0], c3, rig["sync"][0]["c3"])
    x0, y0, x1, y1 = cam.valid_region_left
    ctx.prefetch_staged_pair_sparse(12, 0, True, NF, *PARAMS)
    ctx.sparse_stereo(12, NF, *PARAMS)
    try:
        ctx.set_roi(x0 + 16, y0 + 8, x1, y1)
        a = ctx.sparse_stereo(12, NF, *PARAMS)
        b = ctx.sparse_stereo(22, NF, *PARAMS)
        _same(_slot_arrays(ctx, 12), _slot_arrays(ctx, 22), a, b)
        assert not np.array_equal(_slot_arrays(ctx, 12)["xy"], rig["sync"][0]["xy"])
    finally:
        ctx.set_roi(x0, y0, x1, y1)


def test_orb_into_a_pending_sparse_slot(ctx, rig):
    c, cam, frames = rig["c"], rig["cam"], rig["frames"]
    cam.stage_pairs(frames[:4])
    ctx.prefetch_staged_pair_sparse(6, 1, True, NF, *PARAMS)
    n = ctx.orb_slot_count(6, NF, 0)
    x0, y0, x1, y1 = S.crop_bounds(cam.valid_region_left, c.w, c.h)
    kl = ctx.orb_host(np.ascontiguousarray(frames[1][0][y0:y1, x0:x1]), None, NF)
    got = ctx.download_keypoints(6)
    assert n == len(kl["xy"]) == rig["sync"][1]["c3"][0]
    for k in KP:
        assert np.array_equal(got[k], kl[k]), k
    with pytest.raises(_native.VoError) as e:
        ctx.download_keypoint_depth(6)
    assert e.value.code == VO_E_STATE
    assert ctx.lookahead_depth() == 0
    # ... and the slot's pair is still there: the synchronous call on it
    c3 = ctx.sparse_stereo(6, NF, *PARAMS)
    _same(_slot_arrays(ctx, 6), rig["sync"][1], c3, rig["sync"][1]["c3"])


def test_host_and_host_staged_forms_equal_the_staged_form(ctx, rig):
    L, R = rig["frames"][2]
    ctx.prefetch_pair_sparse(7, L, R, True, NF, *PARAMS)
    w, h, ch = ctx.host_stage_pair(0, L, R)
    ctx.prefetch_host_staged_sparse(8, 0, w, h, ch, True, NF, *PARAMS)
    assert ctx.lookahead_depth() == 2
    for s in (8, 7):
        c3 = ctx.sparse_stereo(s, NF, *PARAMS)
        _same(_slot_arrays(ctx, s), rig["sync"][2], c3, rig["sync"][2]["c3"])
    assert np.array_equal(ctx.download_left(7, L.shape), L) and np.array_equal(ctx.download_left(8, R.shape, right=True), R)
    assert ctx.lookahead_depth() == 0


def test_hostile_requests_enqueue_nothing(ctx, rig):
    cam, frames = rig["cam"], rig["frames"]
    L, R = frames[0]
    cam.stage_pairs(frames[:2])
    w, h, ch = ctx.host_stage_pair(1, L, R)
    assert ctx.lookahead_depth() == 0
    bad = [((NF,) + PARAMS[:3] + (257,), VO_E_ARG), ((NF,) + PARAMS[:3] + (-1,), VO_E_ARG), ((NF, -1.0, 100, 2.0, 75), VO_E_ARG),
           ((NF, 100.0, 100.0, 2.0, 75), VO_E_ARG), ((NF, 4, float("nan"), 2.0, 75), VO_E_ARG), ((NF, 4, float("inf"), 2.0, 75), VO_E_ARG),
           ((NF, 4, 100, -0.5, 75), VO_E_ARG), ((NF, 4, 100, float("nan"), 75), VO_E_ARG), ((501,) + PARAMS, VO_E_CAP), ((-1,) + PARAMS, VO_E_CAP)]
    for req, code in bad:
        for call in (lambda: ctx.prefetch_staged_pair_sparse(9, 0, True, *req), lambda: ctx.prefetch_pair_sparse(9, L, R, True, *req),
                     lambda: ctx.prefetch_host_staged_sparse(9, 1, w, h, ch, True, *req)):
            with pytest.raises(_native.VoError) as e:
                call()
            assert e.value.code == code, (req, e.value)
    for call in (lambda: ctx.prefetch_staged_pair_sparse(28, 0, True, NF, *PARAMS), lambda: ctx.prefetch_staged_pair_sparse(9, 2, True, NF, *PARAMS),
                 lambda: ctx.prefetch_host_staged_sparse(9, _native.VO_NUM_HOST_STAGE, w, h, ch, True, NF, *PARAMS)):
        with pytest.raises(_native.VoError) as e:
            call()
        assert e.value.code == VO_E_ARG
    assert ctx.lookahead_depth() == 0
    # a context that was never given Q
    c2 = _native.Context(0, 640, 480, 64, 500)
    try:
        c2.stage_pairs(frames[:1])
        w2, h2, ch2 = c2.host_stage_pair(0, L, R)
        for call in (lambda: c2.prefetch_staged_pair_sparse(0, 0, True, NF, *PARAMS), lambda: c2.prefetch_pair_sparse(0, L, R, True, NF, *PARAMS),
                     lambda: c2.prefetch_host_staged_sparse(0, 0, w2, h2, ch2, True, NF, *PARAMS)):
            with pytest.raises(_native.VoError) as e:
                call()
            assert e.value.code == VO_E_STATE and "vo_set_Q" in str(e.value)
        assert c2.lookahead_depth() == 0
    finally:
        c2.close()


# ---- pose steps --------------------------------------------------------------------------------------------------------------------
def test_pose_steps_on_collected_slots(ctx, rig):
    """slots 10 / 11 prefetched and collected, slots 24 / 25 filled synchronously (the module's reference): begin / end on the former
    equal the synchronous calls on the latter; a slot that is still pending is refused"""
    cam, frames = rig["cam"], rig["frames"]
    Q = cam.Q
    K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
    cam.stage_pairs(frames[:2])
    for k in range(2):
        ctx.prefetch_staged_pair_sparse(10 + k, k, True, NF, *PARAMS)
    ctx.sparse_stereo(10, NF, *PARAMS)
    with pytest.raises(_native.VoError) as e:
        ctx.pose_pair_begin(10, 11, RATIO, 10, 0.1, 0.02)                     # slot 11 has not been collected
    assert e.value.code == VO_E_STATE
    ctx.sparse_stereo(11, NF, *PARAMS)
    for thr in ((0.0, 0.0), (0.1, 0.02)):
        want = ctx.pose_pair(24, 25, RATIO, 10, *thr)
        got = ctx.pose_pair_end(ctx.pose_pair_begin(10, 11, RATIO, 10, *thr))
        assert want[0][0] >= 50
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    for refine in (0, 3):
        want = ctx.pnp_pair(24, 25, RATIO, K4, ITERS, THR, SEED, refine=refine, want_matches=True)
        got = ctx.pnp_pair_end(ctx.pnp_pair_begin(10, 11, RATIO, K4, ITERS, THR, SEED, refine=refine, want_matches=True), want_matches=True)
        assert want["n"] >= 50
        for k in ("matches", "n", "best_iter", "best_count", "flags", "refine_status", "refine_steps"):
            assert got[k] == want[k], k
        for k in ("Rt", "Rt_refined", "mask", "q", "t"):
            assert np.array_equal(got[k], want[k]), k


# ---- camera / odometer -------------------------------------------------------------------------------------------------------------
def test_submit_sparse_then_compute_sparse(ctx, rig):
    cam, frames = rig["cam"], rig["frames"]
    want = cam.compute_sparse(*frames[3], NF, preprocessed=True)
    sp = cam.submit_sparse(*frames[3], NF, preprocessed=True)
    assert sp.sparse == (NF, 4.0, 100.0, 2.0, 75) and sp.slot is not None and ctx.lookahead_depth() == 1
    with pytest.raises(ValueError):
        cam.compute_3d(sp, None, preprocessed=True)
    got = cam.compute_sparse(sp, None, NF, preprocessed=True)
    assert ctx.lookahead_depth() == 0
    assert len(got[0]) == len(want[0]) == rig["sync"][3]["c3"][2]
    assert np.array_equal(got[0].xy, want[0].xy) and np.array_equal(np.asarray(got[1]), np.asarray(want[1]))
    assert np.array_equal(_bits(np.asarray(got[2])), _bits(np.asarray(want[2]))) and np.array_equal(_bits(np.asarray(got[3])), _bits(np.asarray(want[3])))
    assert np.array_equal(np.asarray(got[4]), np.asarray(want[4]))
    with pytest.raises(ValueError):
        cam.compute_sparse(sp, None, NF, preprocessed=True)                   # consumed
    # released instead of consumed: the slot goes back, and the handle is spent
    sp = cam.submit_sparse(*frames[2], NF, preprocessed=True)
    cam.release_submitted(sp)
    cam.release_submitted(sp)
    assert ctx.lookahead_depth() == 0 and not any(o is _RESERVED for o in cam._slot_owner)
    with pytest.raises(ValueError):
        cam.compute_sparse(sp, None, NF, preprocessed=True)


def _state(odo, ok):
    return (ok, odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy())


def _chain(odo, frames):
    return [_state(odo, odo.update(L, R)) for L, R in frames]


def _equal(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w[:3] and np.array_equal(g[3], w[3]), (k, g[:3], w[:3])


MODES = {"pnp": dict(pose_method="pnp"), "umeyama-clique": dict(rigidity_threshold=0.1, outlier_threshold=0.02)}


@pytest.fixture(scope="module")
def chains(rig):
    """the plain update() chain over the eight frames per mode, computed when first asked for"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _chain(StereoOdometer(rig["cam"], preprocessed_frames=True, depth="sparse", **MODES[name]), rig["frames"])
            assert sum(w[0] for w in cache[name]) >= 6
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(MODES))
def test_run_submits_ahead_and_equals_the_update_chain(ctx, rig, chains, name):
    cam, frames = rig["cam"], rig["frames"]
    want = chains(name)
    odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **MODES[name])
    got = []
    for ok in odo.run(iter(frames), depth=4):
        if not got:
            depth = ctx.lookahead_depth()
            print("%s: %d sparse pairs in flight behind the first result" % (name, depth))
            assert depth >= 1
        got.append(_state(odo, ok))
    _equal(got, want)
    assert ctx.lookahead_depth() == 0 and not any(o is _RESERVED for o in cam._slot_owner)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixture_of_arrays_submitted_and_staged_pairs(ctx, rig, chains, seed):
    cam, frames = rig["cam"], rig["frames"]
    name = "pnp" if seed == 2 else "umeyama-clique"
    kinds = np.random.default_rng(seed).integers(0, 3, len(frames))
    staged = cam.stage_pairs(frames)
    odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **MODES[name])
    submitted = {k: cam.submit_sparse(*frames[k], NF, preprocessed=True) for k in range(len(frames)) if kinds[k] == 1}
    got = []
    for k, (L, R) in enumerate(frames):
        if kinds[k] == 1:
            got.append(_state(odo, odo.update(submitted[k], None)))
        elif kinds[k] == 2:
            got.append(_state(odo, odo.update(staged[k], None)))
        else:
            got.append(_state(odo, odo.update(L, R)))
    print("seed %d (%s): kinds %s" % (seed, name, kinds.tolist()))
    _equal(got, chains(name))
    assert ctx.lookahead_depth() == 0 and not any(o is _RESERVED for o in cam._slot_owner)


def test_closing_the_generator_gives_every_slot_back(ctx, rig, chains):
    cam, frames = rig["cam"], rig["frames"]
    odo = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **MODES["pnp"])
    g = odo.run(iter(frames), depth=4)
    first = [_state(odo, next(g)), _state(odo, next(g))]
    g.close()
    assert not any(o is _RESERVED for o in cam._slot_owner)
    odo.reset_lookahead()
    assert ctx.lookahead_depth() == 0
    _equal(first, chains("pnp")[:2])
    odo2 = StereoOdometer(cam, preprocessed_frames=True, depth="sparse", **MODES["pnp"])
    _equal([_state(odo2, ok) for ok in odo2.run(iter(frames), depth=4)], chains("pnp"))


def test_dense_run_sparse_run_dense_run_on_one_camera(ctx, rig, chains):
    cam, frames = rig["cam"], rig["frames"]
    kw = dict(preprocessed_frames=True, rigidity_threshold=0.1, outlier_threshold=0.02)

    def dense():
        odo = StereoOdometer(cam, **kw)
        return [_state(odo, ok) for ok in odo.run(iter(frames[:5]), depth=4)]
    before = dense()
    odo = StereoOdometer(cam, depth="sparse", **kw)
    _equal([_state(odo, ok) for ok in odo.run(iter(frames), depth=4)], chains("umeyama-clique"))
    _equal(dense(), before)
    assert sum(b[0] for b in before) >= 4
    assert ctx.sgbm_sweep_status() == 0 and ctx.lookahead_depth() == 0


def _failed_sparse_prefetch_body():
    """Body of test_failed_sparse_submission_leaves_the_context_usable: a process of its own against the test-only build of the
    library (libvo355_hooks.so).  VO_FAULT_PREFETCH=n makes the n-th look-ahead submission return a status inside its engine
    scope, after its ingest was enqueued: a status, not a fault."""
    import os
    c = Corridor("C1")
    frames = c.pairs(0, 3)
    os.environ["VO_FAULT_PREFETCH"] = "2"
    ctx = _native.Context(0, 640, 480, 64, 500)
    del os.environ["VO_FAULT_PREFETCH"]
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)
    want = []
    for k in range(3):
        ctx.upload_pair(20 + k, *frames[k], True)
        c3 = ctx.sparse_stereo(20 + k, NF, *PARAMS)
        want.append(dict(_slot_arrays(ctx, 20 + k), c3=c3))
    ctx.prefetch_pair_sparse(0, *frames[0], True, NF, *PARAMS)
    with pytest.raises(_native.VoError) as e:
        ctx.prefetch_pair_sparse(1, *frames[1], True, NF, *PARAMS)
    assert "injected failure" in str(e.value) and ctx.lookahead_depth() == 1
    with pytest.raises(_native.VoError):
        ctx.sparse_stereo(1, NF, *PARAMS)                                      # the slot holds nothing that may be handed out
    # the context still points at its own stream and scratch: a synchronous call is exact ...
    ctx.upload_pair(2, *frames[2], True)
    c3 = ctx.sparse_stereo(2, NF, *PARAMS)
    _same(_slot_arrays(ctx, 2), want[2], c3, want[2]["c3"])
    # ... the same pair submitted again is exact, and so is the pair submitted before the failure
    ctx.prefetch_pair_sparse(1, *frames[1], True, NF, *PARAMS)
    for k in (1, 0):
        c3 = ctx.sparse_stereo(k, NF, *PARAMS)
        _same(_slot_arrays(ctx, k), want[k], c3, want[k]["c3"])
    assert ctx.lookahead_depth() == 0
    ctx.close()
    print("failed-sparse-prefetch body ok")


def test_failed_sparse_submission_leaves_the_context_usable():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "openvo_amd", "libvo355_hooks.so")
    assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
    env = dict(os.environ, VO355_LIB=hooks)
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_sparse_lookahead as t; t._failed_sparse_prefetch_body()"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "failed-sparse-prefetch body ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
