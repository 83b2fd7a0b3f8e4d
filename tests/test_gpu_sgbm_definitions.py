"""csrc/sgbm.hip + sgbm_diag.inc held to what an SGBM result MEANS (tests/sgbm_def.py: every path a whole volume computed from the
border, whole-volume numpy in int64), not to its restatement oracle/src/sgbm.c.  Everything is integer: every comparison is
equality, bit for bit.

    cases         every case of tests/sgbm_def_cases.py through sgbm_compute_host, twice, with the schedule it must take (DIAG /
                  DIAG_RAGGED / UNFUSED) and a healthy sweep: W + E by k_sgbm_we2 / k_sgbm_we / k_sgbm_pair, padded and exact
                  disparity ranges, 1 .. 8 registers per lane, the reverse sweep of MODE_HH, the unfused arm on a pair that
                  stays 80 % valid at uniquenessRatio 100, blockSize 1 .. 11 with minDisparity -16 .. 3, strips of 7 / 11 / 15 waves
    refused       the cases of fewer than 16 rows are refused with VO_E_CAP (the library's floor), nothing is computed
    sweep         uniquenessRatio 0 .. 100 against the definition's winner stage on ONE summed volume: the threshold
                  reciprocal (urM / urAdd of SgbmGeom) for every divisor, and the switch to the unfused arm at 100
    symmetry      no reference: in MODE_HH the disparity of the pair turned upside down is the disparity turned upside down,
                  median and speckle filter included -- on the cases and on a 640 x 200 Corridor C1 crop (D = 64), where the
                  forward and the reverse sweep cross 28 strips
    group         three different members of the 96 x 21 geometry streamed into one sweep group: each equals the definition

The coverage conditions and the sixteen wrong definitions that these comparisons refuse are those of tests/test_sgbm_def.py.
Every test prints its figures.  Shapes are tens of pixels a side: a few launches each."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_inputs                # noqa: E402
import sgbm_def as DEF             # noqa: E402
import sgbm_def_cases as C         # noqa: E402

pytestmark = pytest.mark.gpu

VO_E_CAP = -4


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
    return {C.DIAG: _native.SCHED_DIAG, C.RAGGED: _native.SCHED_DIAG_RAGGED, C.UNFUSED: _native.SCHED_UNFUSED}[c.sched]


def _hold_case(ctx, c):
    L, R = C.images(c)
    t = time.perf_counter()
    want = C.definition(c)[0]["final"]
    dt = time.perf_counter() - t
    C.hold_coverage(c)
    ctx.set_sgbm(c.p, c.mode)
    got = ctx.sgbm_compute_host(L, R)
    again = ctx.sgbm_compute_host(L, R)
    status, schedule = ctx.sgbm_sweep_status(), ctx.sgbm_last_schedule()
    print("%s; schedule %d, %d pixels differ; %.3f s in the definition" % (C.figures(c), schedule, int((got != want).sum()), dt))
    assert status == 0
    assert schedule == _schedule(c), (schedule, c.sched)
    assert got.dtype == want.dtype and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(again, want), int((again != want).sum())


@pytest.mark.parametrize("name", C.GPU_NAMES)
def test_device_equals_the_definition(contexts, name):
    c = C.BY_NAME[name]
    _hold_case(contexts(c.p["numDisparities"]), c)


@pytest.mark.parametrize("name", C.STRIP_NAMES)
def test_strip_widths(name, monkeypatch):
    """VO_DIAG_WAVES is read when a context is made: a context of its own per strip width"""
    from openvo_amd import _native
    c = C.BY_NAME[name]
    monkeypatch.setenv("VO_DIAG_WAVES", str(c.waves))
    ctx = _native.Context(0, 192, 64, 64, 64)
    try:
        _hold_case(ctx, c)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", C.REFUSED_NAMES)
def test_fewer_than_16_rows_are_refused(contexts, name):
    from openvo_amd import _native
    c = C.BY_NAME[name]
    ctx = contexts(c.p["numDisparities"])
    ctx.set_sgbm(c.p, c.mode)
    with pytest.raises(_native.VoError) as err:
        ctx.sgbm_compute_host(*C.images(c))
    assert err.value.code == VO_E_CAP


@pytest.mark.parametrize("mode", [0, 1])
def test_uniqueness_ratio_sweep(contexts, mode):
    from openvo_amd import _native
    c = C.BY_NAME["we2-96x21-m%d" % mode]
    L, R = C.images(c)
    e = DEF.effective(c.p, c.w)
    S = C.definition(c)[0]["S"]
    ctx = contexts(64)
    t_def, wrong, steps, last, valid = 0.0, [], 0, None, []
    for ur in range(101):
        t = time.perf_counter()
        eu = e._replace(ur=ur)
        want = DEF.post(DEF.wta(S, eu, c.w), eu)[1]
        t_def += time.perf_counter() - t
        ctx.set_sgbm(dict(c.p, uniquenessRatio=ur), mode)
        got = ctx.sgbm_compute_host(L, R)
        assert ctx.sgbm_last_schedule() == (_native.SCHED_UNFUSED if ur == 100 else _native.SCHED_DIAG), ur
        if not np.array_equal(got, want):
            wrong.append((ur, int((got != want).sum())))
        steps += last is not None and not np.array_equal(want, last)
        last = want
        valid.append(int((want >= 0).sum()))
    print("mode %d: uniquenessRatio 0 .. 100: the result changes at %d steps, valid pixels %d -> %d -> %d; ratios that differ: %s; "
          "%.2f s in the definition" % (mode, steps, valid[0], valid[50], valid[100], wrong, t_def))
    assert ctx.sgbm_sweep_status() == 0
    assert steps >= 20
    assert not wrong, wrong


def _flip_symmetry(ctx, L, R, p, what):
    ctx.set_sgbm(p, 1)
    a = ctx.sgbm_compute_host(L, R)
    b = ctx.sgbm_compute_host(np.ascontiguousarray(L[::-1]), np.ascontiguousarray(R[::-1]))
    valid = float((a >= p["minDisparity"] * 16).mean())
    print("%s: %.1f %% of the image valid, %d pixels break the symmetry" % (what, 100 * valid, int((a[::-1] != b).sum())))
    assert ctx.sgbm_sweep_status() == 0
    assert np.array_equal(a[::-1], b), int((a[::-1] != b).sum())
    return valid


@pytest.mark.parametrize("name", C.GPU_NAMES)
def test_upside_down_in_mode_hh(contexts, name):
    """(the definition's S has this symmetry with eight paths and lacks it with five: tests/test_sgbm_def.py)"""
    c = C.BY_NAME[name]
    p = dict(c.p)
    if p["speckleWindowSize"] <= 0:
        p["speckleWindowSize"] = 30
    L, R = C.images(c)
    valid = _flip_symmetry(contexts(p["numDisparities"]), L, R, p, name)
    assert valid > 0.1


def test_upside_down_across_many_strips(contexts):
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    L, R = c.pair(4)
    L, R = np.ascontiguousarray(L[:200, :640]), np.ascontiguousarray(R[:200, :640])
    assert L.shape == (200, 640)
    p = c.sgbm_params(1)
    assert p["numDisparities"] == 64 and p["speckleWindowSize"] > 0
    valid = _flip_symmetry(contexts(64), L, R, p, "Corridor C1 pair 4, 640 x 200")
    assert valid > 0.5


def test_one_sweep_group_of_three(contexts):
    from openvo_amd import _native
    cases = [C.BY_NAME[n] for n in C.GROUP_NAMES]
    w, h, p = cases[0].w, cases[0].h, cases[0].p
    want = [C.definition(c)[0]["final"] for c in cases]
    assert not any(np.array_equal(want[i], want[j]) for i in range(3) for j in range(i))      # three different members
    ctx = _native.Context(0, 192, 64, 64, 64)
    try:
        ctx.set_sgbm(p, 0)
        assert ctx.set_sweep_group(3) == 3
        before = ctx.sweep_group_stats()
        for i, c in enumerate(cases):
            ctx.prefetch_pair(2 + i, *C.images(c), True)
            assert ctx.sweep_group_stats()["open"] == (i + 1 if i < 2 else 0)
        after = ctx.sweep_group_stats()
        assert after["full"] - before["full"] == 1 and after["open"] == 0
        for i in reversed(range(3)):
            got = group_inputs.disp16(ctx, 2 + i, w, h)
            print("%s: %d pixels differ" % (C.figures(cases[i]), int((got != want[i]).sum())))
            assert np.array_equal(got, want[i]), (i, int((got != want[i]).sum()))
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()
