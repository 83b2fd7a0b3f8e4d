"""MODE_SGBM_3WAY (mode 2 of vo_set_sgbm: the paths W, E and N; csrc/sgbm.hip + sgbm_vert.inc) held to tests/sgbm_3way_def.py, the
definition stated on tests/sgbm_def.py.  There is no oracle for this mode; everything is integer: every comparison is equality.

    cases         every case of CASES3 through sgbm_compute_host, twice, with the schedule it must take (VERT / VERT_RAGGED /
                  UNFUSED) and a healthy sweep: W + E by k_sgbm_we2 / k_sgbm_we / k_sgbm_pair in front of k_sgbm_vert, D = 16 .. 256
                  (1 .. 8 registers per lane, padded 16 / 48 / 112 and exact), blockSize 1 .. 11 with minDisparity -16 .. 3, the
                  unfused arm at ratio 100, the speckle filter, unclamped sums beyond 32767, 16 rows
    sweep         uniquenessRatio 0 .. 100 against the definition's winner stage on ONE summed volume
    modes         one context, one pair, modes 0 -> 2 -> 1 -> 2 -> 0: nothing of a previous mode's volumes, records or control block
                  leaks into the next
    causality     no reference: with blockSize 1 and no speckle filter the result on the top k rows of a pair equals the result on
                  the whole pair in rows 0 .. k - 3 (see the test for why not k - 2)
    look-ahead    three pairs streamed in mode 2 at sweep-group size 3 join no group; in mode 0 the same three form one
    corridor      a 640 x 200 crop of Corridor C1 pair 4 (72 waves of k_sgbm_vert, speckle filter on)
    refused       mode 3 (MODE_HH4) and -1: VO_E_ARG, the parameters in force stay in force
    camera        StereoCamera with sgbm_params["mode"] = 2: compute_3d against the definition, run() against the update() loop

The coverage conditions and the wrong direction sets these comparisons refuse are those of tests/test_sgbm_3way_def.py.  Every
test prints its figures.  Shapes are tens of pixels a side but for the two corridor tests: a few launches each."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_inputs                # noqa: E402
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402
import sgbm_3way_def as T          # noqa: E402

pytestmark = pytest.mark.gpu

VO_E_ARG = -1


@pytest.fixture(scope="module")
def contexts():
    """one context per maximum D (64, 128, 256), made when first asked for, closed at the end"""
    from openvo_amd import _native
    made = {}

    def get(D):
        top = 64 if D <= 64 else 128 if D <= 128 else 256
        if top not in made:
            made[top] = _native.Context(0, 640 if top == 64 else 320, 200 if top == 64 else 64, top, 64)
        return made[top]
    yield get
    for c in made.values():
        c.close()


def _schedule(c):
    from openvo_amd import _native
    return {T.VERT: _native.SCHED_VERT, T.VERT_RAGGED: _native.SCHED_VERT_RAGGED, T.UNFUSED: _native.SCHED_UNFUSED}[c.sched]


@pytest.mark.parametrize("name", T.NAMES3)
def test_device_equals_the_definition(contexts, name):
    c = T.BY_NAME3[name]
    ctx = contexts(c.p["numDisparities"])
    L, R = C.images(c)
    t = time.perf_counter()
    want = T.definition3(c)[0]["final"]
    dt = time.perf_counter() - t
    T.hold_coverage3(c)
    ctx.set_sgbm(c.p, 2)
    got = ctx.sgbm_compute_host(L, R)
    again = ctx.sgbm_compute_host(L, R)
    status, schedule = ctx.sgbm_sweep_status(), ctx.sgbm_last_schedule()
    print("%s; schedule %d, %d pixels differ; %.3f s in the definition" % (T.figures3(c), schedule, int((got != want).sum()), dt))
    assert status == 0
    assert schedule == _schedule(c), (schedule, c.sched)
    assert got.dtype == want.dtype and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(again, want), int((again != want).sum())


def test_mode_travels_in_the_parameters_too(contexts):
    """sgbm_params["mode"] = 2 is the way StereoCamera passes it (Context.set_sgbm reads the key)"""
    c = T.BY_NAME3["we-40x17"]
    ctx = contexts(16)
    ctx.set_sgbm(dict(c.p, mode=2))
    got = ctx.sgbm_compute_host(*C.images(c))
    assert ctx.sgbm_last_schedule() == _schedule(c)
    assert np.array_equal(got, T.definition3(c)[0]["final"])


def test_uniqueness_ratio_sweep(contexts):
    from openvo_amd import _native
    c = T.BY_NAME3["we2-96x21"]
    L, R = C.images(c)
    e = DEF.effective(c.p, c.w)
    S = T.definition3(c)[0]["S"]
    ctx = contexts(64)
    t_def, wrong, steps, last, valid = 0.0, [], 0, None, []
    for ur in range(101):
        t = time.perf_counter()
        eu = e._replace(ur=ur)
        want = DEF.post(DEF.wta(S, eu, c.w), eu)[1]
        t_def += time.perf_counter() - t
        ctx.set_sgbm(dict(c.p, uniquenessRatio=ur), 2)
        got = ctx.sgbm_compute_host(L, R)
        assert ctx.sgbm_last_schedule() == (_native.SCHED_UNFUSED if ur == 100 else _native.SCHED_VERT), ur
        if not np.array_equal(got, want):
            wrong.append((ur, int((got != want).sum())))
        steps += last is not None and not np.array_equal(want, last)
        last = want
        valid.append(int((want >= 0).sum()))
    print("mode 2: uniquenessRatio 0 .. 100: the result changes at %d steps, valid pixels %d -> %d -> %d; ratios that differ: %s; "
          "%.2f s in the definition" % (steps, valid[0], valid[50], valid[100], wrong, t_def))
    assert ctx.sgbm_sweep_status() == 0
    assert steps >= 20
    assert not wrong, wrong


def test_modes_in_turn_on_one_context(contexts):
    c3 = T.BY_NAME3["we2-96x21"]
    L, R = C.images(c3)
    want = {0: C.definition(C.BY_NAME["we2-96x21-m0"])[0]["final"], 1: C.definition(C.BY_NAME["we2-96x21-m1"])[0]["final"],
            2: T.definition3(c3)[0]["final"]}
    assert not any(np.array_equal(want[a], want[b]) for a in want for b in want if a < b)
    ctx = contexts(64)
    for mode in (0, 2, 1, 2, 0):
        ctx.set_sgbm(c3.p, mode)
        got = ctx.sgbm_compute_host(L, R)
        print("mode %d: %d pixels differ from its definition" % (mode, int((got != want[mode]).sum())))
        assert np.array_equal(got, want[mode]), mode
    assert ctx.sgbm_sweep_status() == 0


def test_rows_do_not_depend_on_rows_below(contexts):
    """W, E and N reach a pixel from its own row and from above only, so with blockSize 1 and the speckle filter off the rows
    below row y enter the result at y in two places alone: the x-Sobel of the prefilter reads row y + 1, and the 3 x 3 median reads
    the raw rows up to y + 1, i.e. image rows up to y + 2.  On the top k rows of a pair (whose row k - 1 replicates itself where the
    whole pair has row k) rows 0 .. k - 3 of the result are therefore those of the whole pair; row k - 2 already is not (the
    definition: 96 x 40, k = 20, seeds 0 - 2: rows 18 and 19 differ, no other; MODE_HH: every row from 2 or 3 on).  The same is
    asked of the definition here, so the property is the definition's and the device only has to equal it."""
    k = 20
    p = C.params(64, bs=1)
    ctx = contexts(64)
    ctx.set_sgbm(p, 2)
    for seed in (0, 1):
        L, R = C.layered(96, 40, 64, 0, seed)
        top = np.ascontiguousarray(L[:k]), np.ascontiguousarray(R[:k])
        whole, part = ctx.sgbm_compute_host(L, R), ctx.sgbm_compute_host(*top)
        rows = np.nonzero((whole[:k] != part).any(axis=1))[0]
        dw, dp = T.compute3(L, R, p)["final"], T.compute3(*top, p)["final"]
        print("seed %d: rows of the top %d that differ from the whole pair's: device %s, definition %s; %.1f %% valid"
              % (seed, k, rows.tolist(), np.nonzero((dw[:k] != dp).any(axis=1))[0].tolist(), 100 * (whole >= 0).mean()))
        assert np.array_equal(dw[:k - 2], dp[:k - 2])
        assert np.array_equal(whole[:k - 2], part[:k - 2]), rows
        assert np.array_equal(whole, dw) and np.array_equal(part, dp)
        assert (whole[:k - 2] >= 0).mean() > 0.1
    assert ctx.sgbm_sweep_status() == 0


def test_lookahead_joins_no_group_in_mode_2():
    from openvo_amd import _native
    cases = [T.BY_NAME3[n] for n in ("we2-96x21", "we2-96x21-s1", "we2-96x21-s2")]
    w, h, p = cases[0].w, cases[0].h, cases[0].p
    want3 = [T.definition3(c)[0]["final"] for c in cases]
    want0 = [C.definition(C.BY_NAME[n])[0]["final"] for n in C.GROUP_NAMES]
    assert not any(np.array_equal(want3[i], want3[j]) for i in range(3) for j in range(i))      # three different members
    ctx = _native.Context(0, 192, 64, 64, 64)
    try:
        ctx.set_sgbm(p, 2)
        assert ctx.set_sweep_group(3) == 3
        before = ctx.sweep_group_stats()
        for i, c in enumerate(cases):
            ctx.prefetch_pair(2 + i, *C.images(c), True)
            assert ctx.sweep_group_stats()["open"] == 0
        assert ctx.sweep_group_stats() == before                       # no group opened, none closed
        for i in reversed(range(3)):
            got = group_inputs.disp16(ctx, 2 + i, w, h)
            print("%s: %d pixels differ" % (T.figures3(cases[i]), int((got != want3[i]).sum())))
            assert np.array_equal(got, want3[i]), (i, int((got != want3[i]).sum()))
        assert ctx.sgbm_last_schedule() == _native.SCHED_VERT
        # ... and MODE_SGBM on the same context still sweeps the three in one launch
        ctx.set_sgbm(p, 0)
        before = ctx.sweep_group_stats()
        for i, n in enumerate(C.GROUP_NAMES):
            ctx.prefetch_pair(2 + i, *C.images(C.BY_NAME[n]), True)
            assert ctx.sweep_group_stats()["open"] == (i + 1 if i < 2 else 0)
        after = ctx.sweep_group_stats()
        assert after["full"] - before["full"] == 1 and after["open"] == 0
        for i in reversed(range(3)):
            got = group_inputs.disp16(ctx, 2 + i, w, h)
            assert np.array_equal(got, want0[i]), (i, int((got != want0[i]).sum()))
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_corridor_crop_equals_the_definition(contexts):
    from openvo_amd import _native
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    L, R = c.pair(4)
    L, R = np.ascontiguousarray(L[:200, :640]), np.ascontiguousarray(R[:200, :640])
    assert L.shape == (200, 640)
    p = c.sgbm_params(2)
    assert p["numDisparities"] == 64 and p["speckleWindowSize"] > 0 and p["mode"] == 2
    t = time.perf_counter()
    info = {}
    d = T.compute3(L, R, p, info)
    dt = time.perf_counter() - t
    ctx = contexts(64)
    ctx.set_sgbm(p)
    got = ctx.sgbm_compute_host(L, R)
    speckle = int((d["final"] != d["median"]).sum())
    print("Corridor C1 pair 4, 640 x 200, mode 2: %.1f %% of the image valid, uniqueness %d, left-right %d, speckle %d; %d pixels differ; "
          "%.2f s in the definition" % (100 * (d["final"] >= 0).mean(), info["uniqueness"], info["left_right"], speckle,
                                        int((got != d["final"]).sum()), dt))
    assert ctx.sgbm_sweep_status() == 0 and ctx.sgbm_last_schedule() == _native.SCHED_VERT
    assert (d["final"] >= 0).mean() > 0.5 and info["uniqueness"] >= 1 and info["left_right"] >= 1 and speckle >= 1
    assert np.array_equal(got, d["final"]), int((got != d["final"]).sum())


def test_other_modes_are_refused_and_change_nothing(contexts):
    from openvo_amd import _native
    c = T.BY_NAME3["we-56x17"]
    ctx = contexts(16)
    ctx.set_sgbm(c.p, 2)
    for mode in (3, -1):
        with pytest.raises(_native.VoError) as err:
            ctx.set_sgbm(dict(c.p, uniquenessRatio=55, blockSize=9), mode)
        assert err.value.code == VO_E_ARG
        assert "MODE_SGBM_3WAY" in str(err.value)                       # the message names the three modes there are
    got = ctx.sgbm_compute_host(*C.images(c))
    assert ctx.sgbm_last_schedule() == _schedule(c)
    assert np.array_equal(got, T.definition3(c)[0]["final"])


def test_stereo_camera_and_odometer_in_mode_2():
    from openvo_amd import StereoCamera, StereoOdometer, _native
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    frames = c.pairs(0, 4)
    p = c.sgbm_params()
    p["mode"] = 2
    ctx = _native.Context(0, 640, 480, 64, 500)
    try:
        cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), p, (c.w, c.h), context=ctx)
        assert cam.stereoSGBM.mode == 2
        _, disp, _ = cam.compute_3d(*frames[0], preprocessed=True)
        got = np.rint(np.asarray(disp) * 16).astype(np.int16)
        assert ctx.sgbm_last_schedule() == _native.SCHED_VERT
        t = time.perf_counter()
        want = T.compute3(*frames[0], p)["final"]
        dt = time.perf_counter() - t
        vr = cam.valid_region_left
        want = want[vr[1]:vr[3], vr[0]:vr[2]]
        print("Corridor C1 pair 0 through compute_3d: %s, %.1f %% valid, %d pixels differ; %.2f s in the definition"
              % (got.shape, 100 * (want >= 0).mean(), int((got != want).sum()) if got.shape == want.shape else -1, dt))
        assert got.shape == want.shape and np.array_equal(got, want)
        assert (want >= 0).mean() > 0.5
        kw = dict(nfeatures=500, rigidity_threshold=0.1, outlier_threshold=0.02, preprocessed_frames=True)
        odo = StereoOdometer(cam, **kw)
        chain = []
        for L, R in frames:
            ok = odo.update(L, R)
            chain.append((ok, np.array(odo.c_T_w, np.float64).copy()))
        odo2 = StereoOdometer(cam, **kw)
        ahead = [(ok, np.array(odo2.c_T_w, np.float64).copy()) for ok in odo2.run(iter(frames), depth=4)]
        print("accepted: update() %s, run() %s; z after four pairs %.4f m" % ([a for a, _ in chain], [a for a, _ in ahead], odo.current_pose()[2, 3]))
        assert [a for a, _ in ahead] == [a for a, _ in chain]
        for (_, a), (_, b) in zip(ahead, chain):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert sum(bool(a) for a, _ in chain) >= 2 and not np.array_equal(chain[-1][1], np.eye(4))
        assert ctx.sgbm_sweep_status() == 0 and ctx.lookahead_depth() == 0
    finally:
        ctx.close()
