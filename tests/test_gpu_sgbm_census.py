"""The census cost (vo_set_sgbm_cost: VO_SGBM_COST_CENSUS; csrc/sgbm_census.inc) held to tests/sgbm_census_def.py, the definition
stated on tests/sgbm_def.py.  There is no oracle for this cost; everything is integer: every comparison is equality.

    cases         every case of CASES_CENSUS through sgbm_compute_host, twice: the final image, a healthy sweep, the schedule the
                  case must take, the cost in force, and C itself cell for cell (vo_sgbm_cost_volume) -- every window, blockSize
                  1 .. 11 with minDisparity -16 .. 3, D = 16 .. 256, the modes 0, 1, 2, the unfused arm, more than one tile of
                  k_census each way, 16 rows under a 9 x 7 window.  Once, the BT C against DEF.cost_volume through the same entry.
    costs         one context, one pair, BT -> census 9 x 7 -> census 3 x 3 -> BT -> census 9 x 7 in modes 0 and 1 (P2 changes with
                  every switch): nothing of a previous front's planes, signatures, P2 row or control block leaks
    invariance    two strictly increasing grey-level tables: the census result is bit-identical, BT's is not
    sweep         uniquenessRatio 0, 10, 50, 99, 100: the winner stage is not new, but at 100 the unfused schedule reads the d2key
                  that the new front has to initialise
    in place      a staged, already rectified pair is read where it lies: k_census leaves the slot's copy (keepL / keepR)
    look-ahead    three census pairs streamed at sweep-group size 3 join no group; BT mode 0 afterwards still forms one
    corridor      a 640 x 200 crop of Corridor C1 pair 4 with sgbm_params(cost=1), speckle filter on
    refused       costs 2 and -1, windows 4 x 4, 11 x 7, 9 x 9: VO_E_ARG, the setting in force stays in force
    misuse        the three new entries with a NULL context, NULL pointers, hostile integers and in the wrong order: a status
    camera        StereoCamera with sgbm_params["cost"] = 1: compute_3d against the definition, run() against the update() loop

The coverage conditions and the wrong variants these comparisons refuse are those of tests/test_sgbm_census_def.py.  Every test
prints its figures.  Shapes are tens of pixels a side but for the two corridor tests: a few launches each."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_inputs                # noqa: E402
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402
import sgbm_census_def as Z        # noqa: E402

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
    return {C.DIAG: _native.SCHED_DIAG, C.RAGGED: _native.SCHED_DIAG_RAGGED, C.UNFUSED: _native.SCHED_UNFUSED,
            Z.T3.VERT: _native.SCHED_VERT, Z.T3.VERT_RAGGED: _native.SCHED_VERT_RAGGED}[c.sched]


def _params(c):
    return dict(c.p, cost=1, censusWidth=c.cw, censusHeight=c.ch)


@pytest.mark.parametrize("name", Z.NAMES)
def test_device_equals_the_definition(contexts, name):
    c = Z.BY_NAME[name]
    ctx = contexts(c.p["numDisparities"])
    L, R = Z.images(c)
    t = time.perf_counter()
    d = Z.definition(c)[0]
    dt = time.perf_counter() - t
    Z.hold_coverage_census(c)
    ctx.set_sgbm(_params(c), c.mode)
    got = ctx.sgbm_compute_host(L, R)
    vol = ctx.sgbm_cost_volume(c.w, c.h)
    again = ctx.sgbm_compute_host(L, R)
    status, schedule = ctx.sgbm_sweep_status(), ctx.sgbm_last_schedule()
    cells = int((vol != d["C"]).sum()) if vol.shape == d["C"].shape else -1
    print("%s; schedule %d, %d cells of C and %d pixels differ; %.3f s in the definition" % (Z.figures(c), schedule, cells, int((got != d["final"]).sum()), dt))
    assert ctx.sgbm_cost() == (1, (c.cw, c.ch))
    assert status == 0
    assert schedule == _schedule(c), (schedule, c.sched)
    assert vol.shape == d["C"].shape and np.array_equal(vol, d["C"]), cells
    assert got.dtype == d["final"].dtype and np.array_equal(got, d["final"]), int((got != d["final"]).sum())
    assert np.array_equal(again, d["final"]), int((again != d["final"]).sum())


def test_bt_cost_volume_through_the_same_entry(contexts):
    c = C.BY_NAME["we2-96x21-m0"]
    ctx = contexts(64)
    L, R = C.images(c)
    ctx.set_sgbm(c.p, 0)
    assert ctx.sgbm_cost() == (0, (9, 7))
    got = ctx.sgbm_compute_host(L, R)
    vol = ctx.sgbm_cost_volume(c.w, c.h)
    want = DEF.cost_volume(L, R, c.p)
    assert np.array_equal(got, C.definition(c)[0]["final"])
    assert vol.shape == want.shape and np.array_equal(vol, want), int((vol != want).sum())


def test_costs_in_turn_on_one_context(contexts):
    c = Z.BY_NAME["we2-96x21-m0"]
    L, R = Z.images(c)
    p_bt = C.params(64)
    p_97, p_33 = dict(c.p, cost=1, censusWidth=9, censusHeight=7), dict(c.p, cost=1, censusWidth=3, censusHeight=3)
    assert p_bt["P2"] != p_97["P2"]                                          # every switch of the cost changes the P2 row behind C too
    ctx = contexts(64)
    for mode in (0, 1):
        want = {"bt": DEF.compute(L, R, p_bt, mode)["final"], "9x7": Z.compute_census(L, R, c.p, mode, 9, 7)["final"],
                "3x3": Z.compute_census(L, R, c.p, mode, 3, 3)["final"]}
        assert not any(np.array_equal(want[a], want[b]) for a in want for b in want if a < b)
        for what, p in (("bt", p_bt), ("9x7", p_97), ("3x3", p_33), ("bt", p_bt), ("9x7", p_97)):
            ctx.set_sgbm(p, mode)
            got = ctx.sgbm_compute_host(L, R)
            print("mode %d, %s: %d pixels differ from its definition" % (mode, what, int((got != want[what]).sum())))
            assert np.array_equal(got, want[what]), (mode, what)
    assert ctx.sgbm_sweep_status() == 0


def test_monotone_grey_level_tables_change_nothing_under_census(contexts):
    (L, R), (L2, R2) = Z.invariance_pairs()
    p_bt = C.params(64)
    p = dict(Z.census_params(p_bt, "layered"), cost=1)
    ctx = contexts(64)
    ctx.set_sgbm(p, 0)
    a, b = ctx.sgbm_compute_host(L, R), ctx.sgbm_compute_host(L2, R2)
    want = Z.compute_census(L, R, p, 0, 9, 7)["final"]
    ctx.set_sgbm(p_bt, 0)
    ba, bb = ctx.sgbm_compute_host(L, R), ctx.sgbm_compute_host(L2, R2)
    print("two monotone tables: census differs in %d pixels, BT in %d of %d" % (int((a != b).sum()), int((ba != bb).sum()), a.size))
    assert np.array_equal(a, want) and np.array_equal(a, b)
    assert not np.array_equal(ba, bb)
    assert ctx.sgbm_sweep_status() == 0


def test_uniqueness_ratio_sweep(contexts):
    from openvo_amd import _native
    c = Z.BY_NAME["double-ur10-m0"]       # (noise-free exact matches: pixels stay valid at ratio 100, so disp2 decides there)
    L, R = Z.images(c)
    e = DEF.effective(c.p, c.w)
    S = Z.definition(c)[0]["S"]
    ctx = contexts(64)
    wrong, valid = [], []
    for ur in (0, 10, 50, 99, 100):
        eu = e._replace(ur=ur)
        want = DEF.post(DEF.wta(S, eu, c.w), eu)[1]
        ctx.set_sgbm(dict(_params(c), uniquenessRatio=ur), c.mode)
        got = ctx.sgbm_compute_host(L, R)
        assert ctx.sgbm_last_schedule() == (_native.SCHED_UNFUSED if ur == 100 else _native.SCHED_DIAG), ur
        if not np.array_equal(got, want):
            wrong.append((ur, int((got != want).sum())))
        valid.append(int((want >= 0).sum()))
    print("census 3 x 7: uniquenessRatio 0, 10, 50, 99, 100: valid pixels %s; ratios that differ: %s" % (valid, wrong))
    assert ctx.sgbm_sweep_status() == 0
    assert valid[0] > valid[-1] > 0                                          # (at 100 a pixel needs disp2, i.e. d2key, to stay valid)
    assert not wrong, wrong


def test_a_pair_read_where_it_lies_leaves_the_slots_copy():
    from openvo_amd import _native
    c = Z.BY_NAME["tiles-200x40"]
    L, R = Z.images(c)
    want = Z.definition(c)[0]["final"]
    ctx = _native.Context(0, 256, 64, 64, 64)
    try:
        ctx.set_sgbm(_params(c), c.mode)
        ctx.stage_pairs([(L, R)])
        for slot in (2, 3):                                                 # (twice: the second run finds the first one's signatures and control block)
            ctx.prefetch_staged_pair(slot, 0, True)
            got = group_inputs.disp16(ctx, slot, c.w, c.h)
            assert np.array_equal(got, want), int((got != want).sum())
            assert np.array_equal(ctx.download_left(slot, L.shape), L)
            assert np.array_equal(ctx.download_left(slot, R.shape, right=True), R)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_lookahead_joins_no_group_under_census():
    from openvo_amd import _native
    cases = [Z.BY_NAME[n] for n in ("we2-96x21-m0", "we2-96x21-s1", "we2-96x21-s2")]
    w, h = cases[0].w, cases[0].h
    # (one setting for the three: the window of the first)
    p = _params(cases[0])
    want1 = [Z.compute_census(*Z.images(c), c.p, 0, cases[0].cw, cases[0].ch)["final"] for c in cases]
    want0 = [C.definition(C.BY_NAME[n])[0]["final"] for n in C.GROUP_NAMES]
    assert not any(np.array_equal(want1[i], want1[j]) for i in range(3) for j in range(i))      # three different members
    ctx = _native.Context(0, 192, 64, 64, 64)
    try:
        ctx.set_sgbm(p, 0)
        assert ctx.set_sweep_group(3) == 3
        before = ctx.sweep_group_stats()
        for i, c in enumerate(cases):
            ctx.prefetch_pair(2 + i, *Z.images(c), True)
            assert ctx.sweep_group_stats()["open"] == 0
        assert ctx.sweep_group_stats() == before                       # no group opened, none closed
        for i in reversed(range(3)):
            got = group_inputs.disp16(ctx, 2 + i, w, h)
            print("%s: %d pixels differ" % (cases[i].name, int((got != want1[i]).sum())))
            assert np.array_equal(got, want1[i]), (i, int((got != want1[i]).sum()))
        assert ctx.sgbm_last_schedule() == _native.SCHED_DIAG
        # ... and BT on the same context still sweeps the three in one launch
        ctx.set_sgbm(C.BY_NAME[C.GROUP_NAMES[0]].p, 0)
        assert ctx.sgbm_cost()[0] == 0
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
    p = c.sgbm_params(cost=1)
    assert p["numDisparities"] == 64 and p["speckleWindowSize"] > 0 and p["cost"] == 1
    t = time.perf_counter()
    info = {}
    d = Z.compute_census(L, R, p, 0, p["censusWidth"], p["censusHeight"], info)
    dt = time.perf_counter() - t
    ctx = contexts(64)
    ctx.set_sgbm(p)
    got = ctx.sgbm_compute_host(L, R)
    speckle = int((d["final"] != d["median"]).sum())
    print("Corridor C1 pair 4, 640 x 200, census 9 x 7: %.1f %% of the image valid, uniqueness %d, left-right %d, speckle %d; %d pixels differ; "
          "%.2f s in the definition" % (100 * (d["final"] >= 0).mean(), info["uniqueness"], info["left_right"], speckle,
                                        int((got != d["final"]).sum()), dt))
    assert ctx.sgbm_sweep_status() == 0 and ctx.sgbm_last_schedule() == _native.SCHED_DIAG
    assert (d["final"] >= 0).mean() > 0.5 and info["uniqueness"] >= 1 and info["left_right"] >= 1 and speckle >= 1
    assert np.array_equal(got, d["final"]), int((got != d["final"]).sum())


def test_other_costs_and_windows_are_refused_and_change_nothing(contexts):
    from openvo_amd import _native
    c = Z.BY_NAME["we-56x17"]
    ctx = contexts(16)
    ctx.set_sgbm(_params(c), c.mode)
    for cost, window in ((2, (9, 7)), (-1, (9, 7)), (1, (4, 4)), (1, (11, 7)), (1, (9, 9))):
        with pytest.raises(_native.VoError) as err:
            ctx.set_sgbm_cost(cost, window)
        assert err.value.code == VO_E_ARG
        assert ctx.sgbm_cost() == (1, (c.cw, c.ch))
    with pytest.raises(_native.VoError) as err:                             # ... and through the parameter dict, with other parameters beside it
        ctx.set_sgbm(dict(c.p, uniquenessRatio=55, blockSize=9, cost=1, censusWidth=9, censusHeight=9), c.mode)
    assert err.value.code == VO_E_ARG
    got = ctx.sgbm_compute_host(*Z.images(c))
    assert ctx.sgbm_last_schedule() == _schedule(c)
    assert np.array_equal(got, Z.definition(c)[0]["final"])
    # BT ignores the window arguments; the native setting outlives vo_set_sgbm
    ctx.set_sgbm_cost(0, (4, 4))
    assert ctx.sgbm_cost()[0] == 0
    ctx.set_sgbm_cost(1, (c.cw, c.ch))
    ctx._ck(ctx._lib.vo_set_sgbm(ctx._h, *[int(c.p[k]) for k in ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
                                                                "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange")], c.mode))
    assert ctx.sgbm_cost() == (1, (c.cw, c.ch))
    assert np.array_equal(ctx.sgbm_compute_host(*Z.images(c)), Z.definition(c)[0]["final"])


def test_the_three_entries_answer_misuse_with_a_status():
    """NULL context, NULL pointers, hostile integers, a volume asked for before any run: a status every time.  The one call that
    may succeed on garbage is cost 0, whose window arguments are ignored by definition -- and it changes nothing."""
    import ctypes
    from openvo_amd import _native
    VO_E_STATE = -3
    ctx = _native.Context(0, 64, 64, 16, 64)
    try:
        L, h = ctx._lib, ctx._h
        ints = [-1, 0, 1, 2, 4, 27, 1000, 2 ** 31 - 1, -2 ** 31]
        buf = (ctypes.c_int16 * 16)()
        three = [ctypes.c_int(-7) for _ in range(3)]
        assert L.vo_set_sgbm_cost(None, 0, 9, 7) == VO_E_ARG and L.vo_set_sgbm_cost(None, 1, 9, 7) == VO_E_ARG
        assert L.vo_get_sgbm_cost(None, *[ctypes.byref(v) for v in three]) == VO_E_ARG and [v.value for v in three] == [-7] * 3
        assert L.vo_sgbm_cost_volume(None, buf, 16) == VO_E_ARG
        for k in range(3):
            args = [ctypes.byref(v) for v in three]
            args[k] = None
            assert L.vo_get_sgbm_cost(h, *args) == VO_E_ARG
        assert L.vo_sgbm_cost_volume(h, None, 0) == VO_E_ARG
        assert L.vo_sgbm_cost_volume(h, buf, 16) == VO_E_STATE          # a fresh context: no run has left a volume
        assert ctx.sgbm_cost() == (0, (9, 7))                           # a fresh context has BT
        ok = 0
        for cost in ints:
            for cw in ints:
                for ch in ints:
                    rc = L.vo_set_sgbm_cost(h, cost, cw, ch)
                    assert rc == (0 if cost == 0 else VO_E_ARG), (cost, cw, ch, rc)
                    ok += rc == 0
                    assert ctx.sgbm_cost() == (0, (9, 7))
        assert ok == len(ints) ** 2
        ctx.set_sgbm(C.params(16))
        ctx.sgbm_compute_host(*C.images(C.BY_NAME["we-40x17"]))
        for cells in (0, 1, 17 * 24 * 16 - 1, 17 * 24 * 16 + 1, 17 * 24 * 32, 2 ** 40):
            assert L.vo_sgbm_cost_volume(h, buf, ctypes.c_size_t(cells)) == VO_E_ARG, cells
        assert ctx.sgbm_cost_volume(40, 17).shape == (17, 24, 16)
    finally:
        ctx.close()


def test_stereo_camera_and_odometer_under_census():
    from openvo_amd import StereoCamera, StereoOdometer, _native
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    frames = c.pairs(0, 4)
    p = c.sgbm_params(cost=1)
    ctx = _native.Context(0, 640, 480, 64, 500)
    try:
        cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), p, (c.w, c.h), context=ctx)
        assert cam.stereoSGBM.cost == 1 and cam.stereoSGBM.census_window == (9, 7) and ctx.sgbm_cost() == (1, (9, 7))
        _, disp, _ = cam.compute_3d(*frames[0], preprocessed=True)
        got = np.rint(np.asarray(disp) * 16).astype(np.int16)
        assert ctx.sgbm_last_schedule() == _native.SCHED_DIAG
        t = time.perf_counter()
        want = Z.compute_census(*frames[0], p, 0, 9, 7)["final"]
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
