"""Sweep groups on the two lane streams.  While the group size in force is above 1 every dense look-ahead submission that may
defer goes on the open group's lane -- ingest, planes, cost volume; the whole chain where only the geometry keeps the run from
deferring -- the group's chain follows on the same lane, and consecutive groups alternate between the lanes.  What remains to
be ordered is an engine that is given work on another stream than the one that carries its latest work: the other lane
(consecutive groups that share engines) or its own stream (sparse and monocular submissions, runs that can never defer, group
size 1).

Every case runs on a fresh context at 224 x 96, D = 32, 300 features, pairs of tests/group_inputs.py, a different pair for every
submission.  Every disparity, and the keypoints and descriptors of the look-ahead ORB, are compared bit for bit with the oracle
and with the same pair streamed at group size 1 (module-wide, on a context of its own: computed once per pair and never
changed).  No case waits on the host between the groups it submits unless it says so; every case ends with
sgbm_sweep_status() == 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Coverage, disp16, pair, params

pytestmark = pytest.mark.gpu

W, H, D, NF = 224, 96, 32, 300
P = params(D)
ORB = (NF, 1, 16, 16 * 24)                       # the fused mask keeps disparities of 1 .. 24 pixels
FIELDS = ("xy", "angle", "octave", "response", "size", "desc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cov(oracle):
    return Coverage(oracle)


@pytest.fixture(scope="module")
def refs(oracle, cov):
    """pair k under parameters p / mode -> (input record, oracle keypoints on the oracle's disparity mask, the pair at group size
    1: keypoints and disparity).  One context for all the runs at group size 1, each pair once."""
    ctx = _native.Context(0, W, H, D, NF, engines=2)
    assert ctx.set_sweep_group(1) == 1
    ctx.lookahead_orb(*ORB)
    memo = {}

    def get(k, p=P, mode=0):
        key = (k, mode) + tuple(sorted(p.items()))
        if key not in memo:
            c = cov.get(W, H, k, p, mode) if mode == 0 and p["uniquenessRatio"] < 100 else cov.entry(W, H, k, p, mode)
            mask = ((c["ref"] >= ORB[2]) & (c["ref"] <= ORB[3])).astype(np.uint8) * 255
            kp = oracle.orb_detect_and_compute(c["L"], mask, NF, cap=2 * NF + 8192)
            ctx.set_sgbm(p, mode)
            ctx.prefetch_pair(3, c["L"], c["R"], True)
            assert ctx.sweep_group_stats()["open"] == 0
            alone = (_keypoints(ctx, 3), disp16(ctx, 3, W, H))
            memo[key] = (c, kp, alone)
        return memo[key]
    yield get
    assert ctx.sgbm_sweep_status() == 0
    ctx.close()


def _keypoints(ctx, slot, request=ORB):
    return {name: v.copy() for name, v in ctx.orb_slot(slot, *request).items()}


def _same(a, b, what):
    for name in FIELDS:
        assert a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint8), np.ascontiguousarray(b[name]).view(np.uint8)), (what, name)


def _check(ctx, slot, ref, what):
    """the slot's disparity and look-ahead keypoints against the oracle and the pair at group size 1, all three ways"""
    c, kp, (kp1, d1) = ref
    got_kp, got = _keypoints(ctx, slot), disp16(ctx, slot, W, H)
    assert np.array_equal(d1, c["ref"]), (what, "alone vs oracle", int((d1 != c["ref"]).sum()))
    assert np.array_equal(got, c["ref"]), (what, "lanes vs oracle", int((got != c["ref"]).sum()))
    assert np.array_equal(got, d1), (what, "lanes vs alone")
    _same(kp1, kp, (what, "alone vs oracle"))
    _same(got_kp, kp, (what, "lanes vs oracle"))
    _same(got_kp, kp1, (what, "lanes vs alone"))


def _context(engines, B):
    ctx = _native.Context(0, W, H, D, NF, engines=engines)
    ctx.set_sgbm(P)
    ctx.lookahead_orb(*ORB)
    assert ctx.set_sweep_group(B) == B
    return ctx


def _closed(ctx):
    st = ctx.sweep_group_stats()
    return st["full"], st["consumer"], st["flush"], st["other"], st["open"]


def test_banks(refs):
    """4 engines, groups of 2: consecutive groups use disjoint engines and alternate lanes.  Three groups back to back with no
    host wait, a fourth after vo_synchronize; nothing is read before all four are submitted."""
    r = [refs(k) for k in range(8)]
    ctx = _context(4, 2)
    try:
        for k in range(6):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert _closed(ctx) == (3, 0, 0, 0, 0)
        ctx.synchronize()
        for k in (6, 7):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert _closed(ctx) == (4, 0, 0, 0, 0)
        for k in reversed(range(8)):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("engines", [3, 4])
def test_engines_shared_by_consecutive_groups(refs, engines):
    """groups of 3 on 3 / 4 engines: every engine is a member of consecutive groups, which lie on different lanes -- its front on
    the new lane waits once for the other lane's chain.  Three groups back to back, nothing read in between."""
    r = [refs(k) for k in range(9)]
    ctx = _context(engines, 3)
    try:
        for k in range(9):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert _closed(ctx) == (3, 0, 0, 0, 0)
        for k in range(9):
            _check(ctx, 2 + (k * 4) % 9, r[(k * 4) % 9], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["mode_hh", "uniqueness_100", "nothing_to_compute"])
def test_runs_that_do_not_defer_between_deferring_pairs(oracle, refs, kind):
    """a run whose whole chain is enqueued at once, between pairs that defer: MODE_HH and uniquenessRatio 100 can never defer
    and keep to their engine's own stream (the setter closes the open group first; the engine leaves the lane and comes back
    to one), a geometry with nothing to compute (W1 <= 0) travels on the lane and passes the open group by"""
    r = [refs(k) for k in range(5)]
    ctx = _context(4, 3)
    try:
        ctx.prefetch_pair(2, r[0][0]["L"], r[0][0]["R"], True)
        assert ctx.sweep_group_stats()["open"] == 1
        if kind == "nothing_to_compute":
            L, R = pair(D, H, 40, D, 0)
            odd = oracle.sgbm_compute(L, R, P, 0)
            ctx.prefetch_pair(9, L, R, True)
            assert _closed(ctx) == (0, 0, 0, 0, 1)
        else:
            p, mode = (P, 1) if kind == "mode_hh" else (params(D, uniquenessRatio=100), 0)
            odd = refs(7, p, mode)
            ctx.set_sgbm(p, mode)
            assert _closed(ctx) == (0, 0, 0, 1, 0)
            ctx.prefetch_pair(9, odd[0]["L"], odd[0]["R"], True)
            assert ctx.sweep_group_stats()["open"] == 0
            ctx.set_sgbm(P)
        for k in (1, 2, 3, 4):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        if kind == "nothing_to_compute":
            assert _closed(ctx) == (1, 0, 0, 0, 2)
            got = disp16(ctx, 9, D, H)
            assert np.array_equal(got, odd) and (got < 0).all()
        else:
            assert _closed(ctx) == (1, 0, 0, 1, 1)
            _check(ctx, 9, odd, kind)
        for k in range(5):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_engine_from_a_sparse_submission_to_a_lane_and_back(refs):
    """2 engines: a sparse look-ahead pair on each engine's own stream, then a group of 2 dense pairs on a lane in the same
    engines' workspaces and ORB scratch, then sparse pairs again.  The sparse results equal those of the same requests on a
    context that never ran anything else."""
    r = [refs(k) for k in range(4)]
    Q = np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 200.0], [0, 0, 10.0, 0]], np.float64)
    req = (NF, 1.0, float(D - 2))

    def sparse(ctx, slot, k):
        ctx.prefetch_pair_sparse(slot, r[k][0]["L"], r[k][0]["R"], True, *req)

    def collect(ctx, slot):
        counts = ctx.sparse_stereo(slot, *req).copy()
        return counts, ctx.download_keypoints(slot), ctx.download_keypoint_depth(slot)

    plain = _native.Context(0, W, H, D, NF, engines=2)
    ctx = _context(2, 2)
    try:
        want = []
        plain.set_Q(Q)
        for k in range(4):
            sparse(plain, 10 + k, k)
        want = [collect(plain, 10 + k) for k in range(4)]
        ctx.set_Q(Q)
        sparse(ctx, 10, 0)
        sparse(ctx, 11, 1)
        ctx.prefetch_pair(2, r[2][0]["L"], r[2][0]["R"], True)
        ctx.prefetch_pair(3, r[3][0]["L"], r[3][0]["R"], True)
        assert _closed(ctx) == (1, 0, 0, 0, 0)
        sparse(ctx, 12, 2)
        sparse(ctx, 13, 3)
        ctx.prefetch_pair(4, r[0][0]["L"], r[0][0]["R"], True)
        ctx.prefetch_pair(5, r[1][0]["L"], r[1][0]["R"], True)
        assert _closed(ctx) == (2, 0, 0, 0, 0)
        for slot, k in ((2, 2), (3, 3), (4, 0), (5, 1)):
            _check(ctx, slot, r[k], ("dense", k))
        for k in range(4):
            counts, kp, (xyz, disp) = collect(ctx, 10 + k)
            assert counts[2] > 20, counts
            assert np.array_equal(counts, want[k][0]), (k, counts, want[k][0])
            _same(kp, want[k][1], ("sparse", k))
            assert np.array_equal(xyz.view(np.uint8), want[k][2][0].view(np.uint8)) and np.array_equal(disp.view(np.uint8), want[k][2][1].view(np.uint8)), k
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()
        plain.close()


def test_engine_from_a_monocular_submission_to_a_lane_and_back(oracle, refs):
    """vo_prefetch_staged_mono runs on engine 0's own stream in engine 0's ORB scratch; the group of 2 that follows uses the same
    scratch on a lane, the monocular extractions behind it engines 1 and 0 on their own streams again"""
    r = [refs(k) for k in range(4)]
    ctx = _context(2, 2)
    try:
        ctx.stage_pairs([(r[k][0]["L"], r[k][0]["R"]) for k in range(4)])
        ctx.prefetch_staged_mono(10, 0, NF)
        ctx.prefetch_pair(2, r[2][0]["L"], r[2][0]["R"], True)
        ctx.prefetch_pair(3, r[3][0]["L"], r[3][0]["R"], True)
        ctx.prefetch_staged_mono(11, 1, NF)
        ctx.prefetch_staged_mono(12, 2, NF)
        ctx.prefetch_pair(4, r[0][0]["L"], r[0][0]["R"], True)
        ctx.prefetch_pair(5, r[1][0]["L"], r[1][0]["R"], True)
        assert _closed(ctx) == (2, 0, 0, 0, 0)
        for slot, k in ((2, 2), (3, 3), (4, 0), (5, 1)):
            _check(ctx, slot, r[k], ("dense", k))
        for k in range(3):
            want = oracle.orb_detect_and_compute(r[k][0]["L"], None, NF, cap=2 * NF + 8192)
            assert len(want["xy"]) > 100
            _same(_keypoints(ctx, 10 + k, (NF, 0, 0, 0)), want, ("mono", k))
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_group_size_one_and_back(refs):
    """vo_set_sweep_group(1): a pair on its engine's own stream; vo_set_sweep_group(2): pairs on the lanes in the same engines;
    and back"""
    r = [refs(k) for k in range(7)]
    ctx = _context(2, 1)
    try:
        ctx.prefetch_pair(2, r[0][0]["L"], r[0][0]["R"], True)
        assert ctx.set_sweep_group(2) == 2
        for k in (1, 2, 3, 4):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert ctx.set_sweep_group(1) == 1
        for k in (5, 6):
            ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert _closed(ctx) == (2, 0, 0, 0, 0)
        for k in range(7):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_host_sources_through_a_group(refs):
    """vo_prefetch_pair from numpy arrays and vo_prefetch_host_staged out of the pinned staging buffers, alternating through two
    groups of 3: the upload and the ingest go on the lane"""
    r = [refs(k) for k in range(6)]
    ctx = _context(4, 3)
    try:
        for k in (1, 3, 5):
            ctx.host_stage_pair(k, r[k][0]["L"], r[k][0]["R"])
        for k in range(6):
            if k % 2:
                ctx.prefetch_host_staged(2 + k, k, W, H, 1, True)
            else:
                ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
        assert _closed(ctx) == (2, 0, 0, 0, 0)
        for k in range(6):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_engine_0_and_the_main_workspace(oracle, refs):
    """3 engines, groups of 2: engine 0 is a member that does not close (group 1: engines 0, 1), a member that closes (group
    2: engines 2, 0) and no member (group 3: engines 1, 2).  A synchronous run on the main stream, which shares engine 0's
    workspace, follows right behind each group."""
    r = [refs(k) for k in range(9)]
    ctx = _context(3, 2)
    try:
        for g in range(3):
            for k in (2 * g, 2 * g + 1):
                ctx.prefetch_pair(2 + k, r[k][0]["L"], r[k][0]["R"], True)
            assert _closed(ctx) == (g + 1, 0, 0, 0, 0)
            c = r[6 + g][0]
            got = ctx.sgbm_compute_host(c["L"], c["R"])
            assert np.array_equal(got, c["ref"]), ("synchronous run behind group", g, int((got != c["ref"]).sum()))
        # ... and in front of engine 0's next member, with the group still open when the run starts
        ctx.prefetch_pair(10, r[6][0]["L"], r[6][0]["R"], True)      # engine 0
        assert _closed(ctx) == (3, 0, 0, 0, 1)
        got = ctx.sgbm_compute_host(r[7][0]["L"], r[7][0]["R"])
        assert _closed(ctx) == (3, 1, 0, 0, 0)
        assert np.array_equal(got, r[7][0]["ref"])
        for k in range(6):
            _check(ctx, 2 + k, r[k], k)
        _check(ctx, 10, r[6], "closed by the synchronous run")
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def _payload():
    """what the off-switch test compares: three groups of 3 on 4 engines, disparities and keypoints of all nine pairs"""
    ctx = _context(4, 3)
    try:
        pairs = [pair(W, H, k, D, 0) for k in range(9)]
        for k, (L, R) in enumerate(pairs):
            ctx.prefetch_pair(2 + k, L, R, True)
        assert _closed(ctx) == (3, 0, 0, 0, 0)
        out = {}
        for k in range(9):
            out["disp%d" % k] = disp16(ctx, 2 + k, W, H)
            for name, v in _keypoints(ctx, 2 + k).items():
                out["%s%d" % (name, k)] = np.ascontiguousarray(v)
        assert ctx.sgbm_sweep_status() == 0
        return out
    finally:
        ctx.close()


def test_off_switch(tmp_path, refs):
    """VO_GROUP_LANES=0 in a fresh process: every engine keeps to its own stream, and every byte is the same"""
    here = _payload()
    for k in range(9):
        assert np.array_equal(here["disp%d" % k], refs(k)[0]["ref"]), k
    out = str(tmp_path / "off.npz")
    child = subprocess.run([sys.executable, "-m", "tests.test_gpu_group_lanes", out], cwd=ROOT, env=dict(os.environ, VO_GROUP_LANES="0"),
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    off = np.load(out)
    assert sorted(off.files) == sorted(here)
    for name in here:
        assert here[name].shape == off[name].shape and np.array_equal(here[name].view(np.uint8), off[name].view(np.uint8)), name


@pytest.mark.parametrize("engines", [2, 3, 5, 16])
def test_automatic_group_size(engines):
    """without a request the size follows the queue budget: 1 with a hardware queue per stream, otherwise half the engines (at
    most 12), so that consecutive groups use disjoint engines"""
    ctx = _native.Context(0, W, H, D, NF, engines=engines)
    try:
        auto = ctx.set_sweep_group(0)
        queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
        want = 1 if queues >= engines + 4 else min(12, max(1, engines // 2))
        assert auto == want, (engines, queues, auto)
        if auto > 1:
            assert auto == min(12, max(1, engines // 2))
    finally:
        ctx.close()


if __name__ == "__main__":
    np.savez(sys.argv[1], **_payload())
