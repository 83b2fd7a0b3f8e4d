"""Sweep groups carry the stages on either side of the diagonal sweep as well: W + E (k_sgbm_we2) and the post filters
(k_sgbm_post_rows, k_ccl_vmerge, k_ccl_sizes, k_ccl_apply) of all members run as ONE launch each, the member picked by a block
index out of a table in the kernel arguments.  Whatever group a pair travels in, its int16 disparity equals the oracle's SGBM of
that pair and the same pair swept alone (group size 1), bit for bit.  Every member of a group gets a different pair, so a
swapped table entry cannot pass."""
import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Refs, check, pair, params

pytestmark = pytest.mark.gpu

SLOT0 = 2


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0, 192, 64, 64, 500)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(oracle):
    """oracle disparity and the disparity of the pair swept alone, once per (shape, parameters, pair); the oracle's output must
    show that the pair is mostly valid and that both post filters removed pixels (group_inputs.Coverage)"""
    return Refs(oracle)


def _prepare(ctx, refs, jobs, p):
    """references first (they change the group size), then the parameters and the group size of the run under test"""
    for (w, h) in dict.fromkeys((w, h) for (w, h, _) in jobs):       # (what holds per group: for the members of each shape)
        refs.cov.group(w, h, [k for (jw, jh, k) in jobs if (jw, jh) == (w, h)], p)
    want = [refs.get(ctx, w, h, k, p) for (w, h, k) in jobs]
    ctx.set_sgbm(p)
    return want


def _run_group(ctx, refs, w, h, p, B, first=0):
    """B different pairs of one shape submitted back to back: the B-th fills the group, which closes at once"""
    jobs = [(w, h, first + i) for i in range(B)]
    want = _prepare(ctx, refs, jobs, p)
    assert ctx.set_sweep_group(B) == B
    before = ctx.sweep_group_stats()
    for i, (_, _, k) in enumerate(jobs):
        ctx.prefetch_pair(SLOT0 + i, *pair(w, h, k, p["numDisparities"]), True)
        assert ctx.sweep_group_stats()["open"] == (i + 1 if B > 1 and i + 1 < B else 0)
    after = ctx.sweep_group_stats()
    assert after["full"] - before["full"] == (1 if B > 1 else 0) and after["open"] == 0
    for i in reversed(range(B)):                                       # (read in another order than submitted)
        check(ctx, want[i], SLOT0 + i, w, h, (w, h, B, i))
    assert ctx.sgbm_sweep_status() == 0


@pytest.mark.parametrize("speckle", [150, 0])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 12])
def test_cut_row_geometry_every_group_size(ctx, refs, B, speckle):
    """160 x 50, D = 64: W1 = 96 takes k_sgbm_we2; 50 rows are 13 row groups -- the last workgroup of W + E holds a dead group
    behind its barrier -- and a ragged last block of post rows.  With and without the speckle filter's three launches."""
    _run_group(ctx, refs, 160, 50, params(64, speckle), B)


def test_padded_disparity_range(ctx, refs):
    """144 x 50, D = 48: Dp = 64, the padded instantiation; W1 = 96"""
    _run_group(ctx, refs, 144, 50, params(48), 3)


@pytest.mark.parametrize("w", [168, 164])
def test_widths_whose_w_plus_e_stays_with_the_member(ctx, refs, w):
    """W1 = 104 (k_sgbm_we) and W1 = 100 (k_sgbm_pair): W + E runs per member with its front; the post filters still batch"""
    _run_group(ctx, refs, w, 40, params(64), 3)


def test_groups_closed_by_a_consumer_by_a_flush_and_by_a_geometry_change(ctx, refs):
    p = params(64)
    w, h = 160, 50
    # a consumer after 2 of 4 members
    want = _prepare(ctx, refs, [(w, h, 3), (w, h, 4)], p)
    assert ctx.set_sweep_group(4) == 4
    s0 = ctx.sweep_group_stats()
    ctx.prefetch_pair(SLOT0, *pair(w, h, 3), True)
    ctx.prefetch_pair(SLOT0 + 1, *pair(w, h, 4), True)
    assert ctx.sweep_group_stats()["open"] == 2
    check(ctx, want[0], SLOT0, w, h, "consumer 0")
    s1 = ctx.sweep_group_stats()
    assert s1["consumer"] - s0["consumer"] == 1 and s1["open"] == 0
    check(ctx, want[1], SLOT0 + 1, w, h, "consumer 1")
    # lookahead_flush after 3 of 4
    want = _prepare(ctx, refs, [(w, h, k) for k in (5, 6, 7)], p)
    assert ctx.set_sweep_group(4) == 4
    for i, k in enumerate((5, 6, 7)):
        ctx.prefetch_pair(SLOT0 + i, *pair(w, h, k), True)
    assert ctx.sweep_group_stats()["open"] == 3
    ctx.lookahead_flush()
    s2 = ctx.sweep_group_stats()
    assert s2["flush"] - s1["flush"] == 1 and s2["open"] == 0
    for i, k in enumerate((5, 6, 7)):
        check(ctx, want[i], SLOT0 + i, w, h, ("flush", i))
    # the geometry changes in mid-stream: two pairs of 160 x 50, then two of 176 x 50 (W1 = 112, k_sgbm_we2 as well) --
    # the third submission closes the first group, the two geometries never share a launch
    jobs = [(160, 50, 8), (160, 50, 9), (176, 50, 0), (176, 50, 1)]
    want = _prepare(ctx, refs, jobs, p)
    assert ctx.set_sweep_group(4) == 4
    s3 = ctx.sweep_group_stats()
    for i, (jw, jh, k) in enumerate(jobs):
        ctx.prefetch_pair(SLOT0 + i, *pair(jw, jh, k), True)
        assert ctx.sweep_group_stats()["open"] == (1, 2, 1, 2)[i]
    s4 = ctx.sweep_group_stats()
    assert s4["other"] - s3["other"] == 1 and s4["full"] == s3["full"]
    ctx.lookahead_flush()
    assert ctx.sweep_group_stats()["open"] == 0
    for i, (jw, jh, k) in enumerate(jobs):
        check(ctx, want[i], SLOT0 + i, jw, jh, ("geometry", i))
    assert ctx.sgbm_sweep_status() == 0


def test_main_workspace_member_then_a_synchronous_run_at_once(oracle, ctx, refs):
    """Look-ahead engine 0 works in the main workspace.  Its member's run ends with the group's post launches on the closing
    member's stream; a synchronous run on the main stream, started right behind the close, must wait for exactly that -- with
    engine 0's member a non-closing one (engines 0, 1) and the closing one (engines 2, 0)."""
    p = params(64)
    w, h = 160, 50
    c = _native.Context(0, 192, 64, 64, 500, engines=3)                # a fresh context: its first pair goes to engine 0
    try:
        want = _prepare(ctx, refs, [(w, h, k) for k in (0, 1, 2, 3)], p)     # (references on the module's context)
        sync = [pair(w, h, 10), pair(w, h, 11)]
        sync_ref = [oracle.sgbm_compute(L, R, p, 0) for (L, R) in sync]
        c.set_sgbm(p)
        assert c.set_sweep_group(2) == 2
        c.prefetch_pair(SLOT0, *pair(w, h, 0), True)                  # engine 0
        c.prefetch_pair(SLOT0 + 1, *pair(w, h, 1), True)              # engine 1 closes
        assert c.sweep_group_stats()["open"] == 0
        got_sync0 = c.sgbm_compute_host(*sync[0])
        c.prefetch_pair(SLOT0 + 2, *pair(w, h, 2), True)              # engine 2
        c.prefetch_pair(SLOT0 + 3, *pair(w, h, 3), True)              # engine 0 closes
        assert c.sweep_group_stats()["open"] == 0
        got_sync1 = c.sgbm_compute_host(*sync[1])
        assert c.sweep_group_stats()["full"] == 2
        assert np.array_equal(got_sync0, sync_ref[0]) and np.array_equal(got_sync1, sync_ref[1])
        for i in range(4):
            check(c, want[i], SLOT0 + i, w, h, ("engine 0", i))
        assert c.sgbm_sweep_status() == 0
    finally:
        c.close()
