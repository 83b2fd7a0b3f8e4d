"""Sweep groups across the parameter space: every register count of the batched W + E and sweep launches (NP = Dp / 32 =
1 .. 8, padded and unpadded), the smallest cut row, the minimum image height, a minDisparity on either side of 0, more rows than
the CCL grid has blocks, fewer post rows per block than 6, an image too wide for k_sgbm_post_rows (W + E and the sweep batched,
the post passes per member), the extremes of uniquenessRatio and of the speckle filter, and a seeded fuzz over everything
vo_set_sgbm takes.  Every member of a group is a different pair (tests/group_inputs.py: the oracle shows that the post filters
remove pixels of it); its disparity equals the oracle's and the same pair streamed with group size 1, bit for bit."""
import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Refs, check, pair, params

pytestmark = pytest.mark.gpu

SLOT0 = 2
SLOT1 = 14                  # a second group on one context fills other slots: nothing in them to inherit


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


class _Ctx:
    """a context sized to one shape, with as many look-ahead engines as the largest group of the case"""

    def __init__(self, w, h, D, engines):
        self.args = (0, w, max(h, 64), D, 64)
        self.engines = engines

    def __enter__(self):
        self.c = _native.Context(*self.args, engines=self.engines)
        return self.c

    def __exit__(self, *exc):
        self.c.close()


def _run_group(ctx, refs, w, h, p, B, first=0, mode=0, fuzz=False, slot0=SLOT0):
    """B different pairs of one shape submitted back to back.  Where the parameters let a pair wait for its group (MODE_SGBM,
    uniquenessRatio < 100) the B-th fills the group, which closes at once: one `full` closure.  Otherwise nothing is ever open
    and no closure is counted."""
    ks = [first + i for i in range(B)]
    want = refs.group(ctx, w, h, ks, p, mode, fuzz)
    members = [refs.cov.get(w, h, k, p, mode, fuzz) for k in ks]
    ctx.set_sgbm(p, mode)
    assert ctx.set_sweep_group(B) == B
    defers = B > 1 and mode == 0 and 0 <= p["uniquenessRatio"] < 100
    before = ctx.sweep_group_stats()
    for i, m in enumerate(members):
        ctx.prefetch_pair(slot0 + i, m["L"], m["R"], True)
        assert ctx.sweep_group_stats()["open"] == (i + 1 if defers and i + 1 < B else 0)
    after = ctx.sweep_group_stats()
    assert after["open"] == 0
    assert {k: after[k] - before[k] for k in ("full", "consumer", "flush", "other")} == dict(full=1 if defers else 0, consumer=0, flush=0, other=0)
    for i in reversed(range(B)):                                       # (read in another order than submitted)
        check(ctx, want[i], slot0 + i, w, h, (w, h, p, mode, B, i))
    assert ctx.sgbm_sweep_status() == 0


@pytest.mark.parametrize("D", [32, 64, 96, 128, 160, 192, 224, 256])
def test_every_register_count_unpadded(refs, D):
    """(D + 96) x 21, Dp = D: NP = 1 .. 8 of we2_launch_jobs<NP> and launch_diag_k<NP, false, 11 | 7, ...> with 2 and with 5 jobs
    (W1 = 96: the cut row)"""
    w, h = D + 96, 21
    with _Ctx(w, h, D, 5) as ctx:
        for B, slot0 in ((2, SLOT0), (5, SLOT1)):
            _run_group(ctx, refs, w, h, params(D), B, slot0=slot0)


@pytest.mark.parametrize("D", [16, 48, 112, 176, 240])
def test_padded_instantiations(refs, D):
    """Dp = 32, 64, 128, 192, 256 above D: the padded instantiations, three jobs"""
    w, h = D + 96, 21
    with _Ctx(w, h, D, 3) as ctx:
        _run_group(ctx, refs, w, h, params(D), 3)


@pytest.mark.parametrize("w,h,D", [(96, 16, 64), (64, 16, 32), (288, 16, 256)])
def test_smallest_cut_row_at_the_minimum_height(refs, w, h, D):
    """W1 = 32: two 8-column segments per half row of k_sgbm_we2; 16 rows are the least an image may have.  2 and 12 jobs."""
    with _Ctx(w, h, D, 12) as ctx:
        for B, slot0 in ((2, SLOT0), (12, SLOT1)):
            _run_group(ctx, refs, w, h, params(D), B, slot0=slot0)


@pytest.mark.parametrize("w,h,D,minD", [(144, 24, 112, -16), (151, 33, 32, 7), (200, 30, 64, -1)])
def test_min_disparity_on_either_side_of_zero(refs, w, h, D, minD):
    """minDisparity < 0 takes columns off the right end of the band (W1 = 32, 136), > 0 moves its left end (W1 = 112)"""
    with _Ctx(w, h, D, 3) as ctx:
        _run_group(ctx, refs, w, h, params(D, minD=minD), 3)


@pytest.mark.parametrize("w,h,D", [(176, 133, 128), (208, 130, 96)])
def test_more_rows_than_the_ccl_grid(refs, w, h, D):
    """h > 128: the blocks of k_ccl_vmerge / k_ccl_sizes stride over the rows, for every member of 3 and of 12"""
    with _Ctx(w, h, D, 12) as ctx:
        for B, slot0 in ((3, SLOT0), (12, SLOT1)):
            _run_group(ctx, refs, w, h, params(D), B, slot0=slot0)


def test_three_post_rows_per_block_and_a_ragged_last_block(refs):
    """4288 x 20: k_sgbm_post_rows holds rb = 3 rows per block, 7 blocks per member, the last with 2 rows"""
    w, h, D = 4288, 20, 16
    with _Ctx(w, h, D, 3) as ctx:
        _run_group(ctx, refs, w, h, params(D), 3)


def test_too_wide_for_the_fused_post_kernel(oracle, refs):
    """8704 x 16: W + E and the sweep of all members are one launch each, but every member runs its own post passes on its own
    stream behind them.  Three engines, the references at group size 1 taken first (three submissions: the round robin is back at
    engine 0): groups of 2 (engines 0, 1: engine 0's member a non-closing one), 2 (engines 2, 0: the closing one), 1 (engine 1)
    and 3 (engines 2, 0, 1), each followed at once by a synchronous run in the main workspace, which engine 0 shares."""
    w, h, D = 8704, 16, 16
    p = params(D)
    sync = [dict(zip("LR", pair(w, h, k, D))) for k in (8, 9, 10, 11)]
    for s in sync:
        s["ref"] = oracle.sgbm_compute(s["L"], s["R"], p, 0)
    with _Ctx(w, h, D, 3) as ctx:
        refs.group(ctx, w, h, [0, 1, 2], p)
        for i, (B, first, slot0) in enumerate([(2, 0, 2), (2, 1, 4), (1, 0, 6), (3, 0, 7)]):     # (every group fills slots of its own)
            _run_group_then_sync(ctx, refs, w, h, p, B, first, slot0, sync[i])
            assert ctx.sgbm_last_schedule() == _native.SCHED_DIAG


def _run_group_then_sync(ctx, refs, w, h, p, B, first, slot0, sync):
    ks = [first + i for i in range(B)]
    want = refs.group(ctx, w, h, ks, p)
    members = [refs.cov.get(w, h, k, p) for k in ks]
    ctx.set_sgbm(p)
    assert ctx.set_sweep_group(B) == B
    before = ctx.sweep_group_stats()
    for i, m in enumerate(members):
        ctx.prefetch_pair(slot0 + i, m["L"], m["R"], True)
    after = ctx.sweep_group_stats()
    assert after["full"] - before["full"] == (1 if B > 1 else 0) and after["open"] == 0
    assert ctx.sgbm_last_schedule() == _native.SCHED_DIAG
    got = ctx.sgbm_compute_host(sync["L"], sync["R"])
    assert np.array_equal(got, sync["ref"]), ("synchronous run behind the group", B, int((got != sync["ref"]).sum()))
    for i in range(B):
        check(ctx, want[i], slot0 + i, w, h, (w, h, B, i))
    assert ctx.sgbm_sweep_status() == 0


@pytest.mark.parametrize("over", [dict(uniquenessRatio=99), dict(uniquenessRatio=0), dict(speckleWindowSize=100000), dict(speckleRange=0)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_extremes_of_the_uniqueness_test_and_of_the_speckle_filter(refs, over):
    """uniquenessRatio 99 (the reciprocal of 100 - ur is the special case 1) and 0 (no test); a speckle window above the image
    size (every pixel goes) and speckleRange 0.  160 x 50, D = 64, three members."""
    with _Ctx(160, 50, 64, 3) as ctx:
        _run_group(ctx, refs, 160, 50, params(64, **over), 3)


@pytest.mark.parametrize("mode,ur", [(1, 10), (0, 100)], ids=["MODE_HH", "uniquenessRatio100"])
def test_parameters_under_which_no_pair_waits_for_a_group(refs, mode, ur):
    """group size 3, but MODE_HH and the unfused schedule never defer: nothing open after any submission, no closure counted"""
    with _Ctx(160, 50, 64, 3) as ctx:
        _run_group(ctx, refs, 160, 50, params(64, uniquenessRatio=ur), 3, mode=mode)


def _accepted(p):
    """what vo_set_sgbm takes: a path cost must fit the int16 OpenCV computes in"""
    ftzero = max(p["preFilterCap"], 15) | 1
    P1 = p["P1"] if p["P1"] > 0 else 2
    P2 = max(p["P2"] if p["P2"] > 0 else 5, P1 + 1)
    side = p["blockSize"]
    return side <= 11 and P2 <= 8000 and side * side * (2 * ftzero + 63) + P2 <= 32767


N_DRAWS = 8


@pytest.mark.parametrize("seed", [41, 42])
def test_parameter_fuzz_through_groups(refs, seed):
    """what test_sgbm_parameter_fuzz_against_the_oracle draws (MODE_SGBM), every draw a group of 2, 3, 5 or 12 different pairs.
    Drawn inside what vo_set_sgbm accepts -- no refusal --, where a pair waits for its group (uniquenessRatio < 100) and where
    at least half of the computed band is valid in the oracle's disparity of every member under the drawn parameters; all
    decided on the host, from the parameters and the oracle alone, before the context sees the draw."""
    rng = np.random.default_rng(seed)
    with _Ctx(257, 50, 128, 12) as ctx:
        done = 0
        while done < N_DRAWS:
            w = int(rng.choice([150, 176, 200, 257])); h = int(rng.choice([16, 33, 50]))
            D = int(rng.choice([16, 32, 48, 64, 96, 128]))
            mind = int(rng.choice([-32, -1, 0, 0, 7, 40]))
            P1 = int(rng.choice([0, 1, 8, 200, 1000]))
            p = dict(minDisparity=mind, numDisparities=D, blockSize=int(rng.choice([1, 3, 5, 5, 7, 9, 11])), P1=P1,
                     P2=min(8000, P1 + int(rng.choice([0, 1, 24, 600, 3000, 7000]))), disp12MaxDiff=int(rng.choice([-1, 0, 1, 5, 1000])),
                     preFilterCap=int(rng.choice([0, 1, 15, 31, 63, 100, 127])), uniquenessRatio=int(rng.choice([0, 5, 15, 50, 99, 100])),
                     speckleWindowSize=int(rng.choice([0, 10, 100, 100000])), speckleRange=int(rng.choice([0, 1, 2, 10, 100])))
            B = int(rng.choice([2, 3, 5, 12]))
            if w - D < 32 or not _accepted(p) or p["uniquenessRatio"] >= 100:      # (100 never defers: it has a test of its own)
                continue
            if any(refs.cov.entry(w, h, k, p, fuzz=True)["share"] < 0.5 for k in range(B)):
                continue
            _run_group(ctx, refs, w, h, p, B, fuzz=True)
            done += 1
