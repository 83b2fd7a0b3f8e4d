"""vo_get_stage_timeline: the stage timers' brackets one by one (stage, entries, begin, end) -- nothing while timing is off;
with timing on, the brackets of three synchronous pairs in the order they were opened, begin <= end, the stage ids those of
vo_get_timings, and per stage the same total as timings() reports for the same brackets (the accessor consumes nothing)."""
import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import pair, params

pytestmark = pytest.mark.gpu


def test_timeline_matches_timings():
    w, h, D = 224, 96, 64
    ctx = _native.Context(0, w, h, D, 300)
    try:
        ctx.set_sgbm(params(D))

        def one(k):
            ctx.upload_pair(2, *pair(w, h, k, D), True)
            ctx.sgbm_compute(2)
            return ctx.orb_slot(2, 300, 1, 16, 640)

        one(0)
        assert ctx.stage_timeline() == []                               # timing is off: nothing was recorded
        ctx.enable_timing(True)
        for k in (1, 2, 3):
            assert len(one(k)["xy"]) >= 100
        tl = ctx.stage_timeline()
        assert tl == ctx.stage_timeline()                               # (asking consumes nothing)
        t = ctx.timings(reset=True)
        assert ctx.stage_timeline() == []                               # timings() has resolved them
        assert len(tl) >= 3 * 5                                         # cost, W + E, sweep, post filters, ORB of every pair
        assert tl[0][2] == 0.0
        per = {}
        for (stage, entries, begin, end) in tl:
            assert stage in _native.T_STAGES and entries == 1 and begin <= end, (stage, entries, begin, end)
            ms, n = per.get(stage, (0.0, 0))
            per[stage] = (ms + (end - begin), n + entries)
        for stage in ("sgbm_cost", "sgbm_agg", "sgbm_wta", "sgbm_post", "orb"):
            assert per[stage][1] == 3, (stage, per[stage])
        for stage, (ms, n) in t.items():
            got_ms, got_n = per.get(stage, (0.0, 0))
            assert got_n == n and abs(got_ms - ms) <= 1e-3 * max(n, 1), (stage, (got_ms, got_n), (ms, n))
        ctx.enable_timing(False)
        one(4)
        assert ctx.stage_timeline() == []
    finally:
        ctx.close()
