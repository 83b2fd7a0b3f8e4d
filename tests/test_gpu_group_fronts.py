"""Sweep groups whose members leave their fronts -- planes and cost volume -- to the group: with VO_GROUP_FRONTS = F >= 2 a dense
look-ahead run that becomes a member of the open group on a lane launches no front of its own; F pending members' fronts, or
however many are pending when the group closes, go in one k_sgbm_planes and one cost launch (FrontJobs, the member a grid
dimension).  A run that cannot defer -- MODE_HH, uniquenessRatio 100, a geometry that is not k_sgbm_we2's -- launches its
front at once through the same kernels with a table of one.

Every case runs on a fresh context at 224 x 96, D = 32, 300 features unless it says otherwise, pairs of tests/group_inputs.py, a
different pair for every submission.  Every disparity, and the keypoints and descriptors of the look-ahead ORB, are compared
bit for bit with the oracle and with the same pair streamed at group size 1 (module-wide, on a context of its own: computed
once per pair and never changed).  That batching happened is read from the stage timeline: the `entries` of a sgbm_cost
bracket is the number of members its launches carried.  Every case ends with sgbm_sweep_status() == 0.

blockSize 13 (k_sgbm_cost_generic) cannot be reached: vo_set_sgbm refuses every blockSize above 11, so no caller launches that
kernel.  test_block_13_is_refused pins the refusal; the largest block that runs, 11, goes through a batch instead."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Coverage, disp16, pair, params

pytestmark = pytest.mark.gpu

W, H, D, NF = 224, 96, 32, 300
WMAX, DMAX = 352, 160                            # the widest and deepest variant (D = 160: two waves per cost workgroup)
P = params(D)
ORB = (NF, 1, 16, 16 * 24)                       # the fused mask keeps disparities of 1 .. 24 pixels
FIELDS = ("xy", "angle", "octave", "response", "size", "desc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strip_kinds(w, p):
    """(interior, border): how many (strip, wave) of one tile row of k_sgbm_cost_sweep<8, SW> take the staged path and how many
    the shift-chain path -- the kernel's own condition: every column of the strip and its halo inside the computed band, every
    lane's right-image position inside the row"""
    minD, Dn, sw = p["minDisparity"], p["numDisparities"], p["blockSize"] // 2
    minX1 = max(minD + Dn, 0)
    W1 = w + min(minD, 0) - minX1
    XT, NC = 8, 8 + 2 * sw
    NJ = 64 + (NC - 1) // 2
    waves = (((Dn + 31) // 32 * 32) // 2 + 63) // 64
    interior = border = 0
    for xa in range(0, W1, XT):
        for wv in range(waves):
            pmin = xa - sw + minX1 - minD - 128 * wv - 126
            if xa >= sw and xa - sw + NC <= W1 and pmin >= 0 and pmin + 2 * NJ <= w:
                interior += 1
            else:
                border += 1
    return interior, border


def test_the_width_gives_interior_and_border_strips():
    interior, border = strip_kinds(W, P)
    assert interior >= 4 and border >= 4, (interior, border)
    assert (W - D) % 16 == 0 and W - D >= 32                     # k_sgbm_we2's geometry: the runs defer


@pytest.fixture(scope="module")
def cov(oracle):
    return Coverage(oracle)


@pytest.fixture(scope="module")
def refs(oracle, cov):
    """pair k of width w under parameters p / mode -> (input record, oracle keypoints on the oracle's disparity mask, the pair at
    group size 1: keypoints and disparity).  One context for all the runs at group size 1, each pair once."""
    ctx = _native.Context(0, WMAX, H, DMAX, NF, engines=2)
    assert ctx.set_sweep_group(1) == 1
    ctx.lookahead_orb(*ORB)
    memo = {}

    def get(k, p=P, mode=0, w=W):
        key = (k, mode, w) + tuple(sorted(p.items()))
        if key not in memo:
            c = cov.get(w, H, k, p, mode) if mode == 0 and p["uniquenessRatio"] < 100 else cov.entry(w, H, k, p, mode)
            mask = ((c["ref"] >= ORB[2]) & (c["ref"] <= ORB[3])).astype(np.uint8) * 255
            kp = oracle.orb_detect_and_compute(c["L"], mask, NF, cap=2 * NF + 8192)
            ctx.set_sgbm(p, mode)
            ctx.prefetch_pair(3, c["L"], c["R"], True)
            assert ctx.sweep_group_stats()["open"] == 0
            alone = (_keypoints(ctx, 3), disp16(ctx, 3, w, H))
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


def _check(ctx, slot, ref, what, w=W):
    """the slot's disparity and look-ahead keypoints against the oracle and the pair at group size 1, all three ways"""
    c, kp, (kp1, d1) = ref
    got_kp, got = _keypoints(ctx, slot), disp16(ctx, slot, w, H)
    assert np.array_equal(d1, c["ref"]), (what, "alone vs oracle", int((d1 != c["ref"]).sum()))
    assert np.array_equal(got, c["ref"]), (what, "batched vs oracle", int((got != c["ref"]).sum()))
    assert np.array_equal(got, d1), (what, "batched vs alone")
    _same(kp1, kp, (what, "alone vs oracle"))
    _same(got_kp, kp, (what, "batched vs oracle"))
    _same(got_kp, kp1, (what, "batched vs alone"))


def _context(engines, B, F, p=P, w=W, d=D):
    """a fresh context with VO_GROUP_FRONTS = F (read once, by vo_create), every stage timed"""
    before = os.environ.get("VO_GROUP_FRONTS")
    os.environ["VO_GROUP_FRONTS"] = str(F)
    try:
        ctx = _native.Context(0, w, H, d, NF, engines=engines)
    finally:
        if before is None:
            del os.environ["VO_GROUP_FRONTS"]
        else:
            os.environ["VO_GROUP_FRONTS"] = before
    ctx.set_sgbm(p)
    ctx.lookahead_orb(*ORB)
    assert ctx.set_sweep_group(B) == B
    ctx.enable_timing(True)
    return ctx


def _closed(ctx):
    st = ctx.sweep_group_stats()
    return st["full"], st["consumer"], st["flush"], st["other"], st["open"]


def _cost_entries(ctx):
    """`entries` of every sgbm_cost bracket so far, in the order the launches were enqueued"""
    return [n for (stage, n, _, _) in ctx.stage_timeline() if stage == "sgbm_cost"]


def _put(ctx, slot, ref):
    ctx.prefetch_pair(slot, ref[0]["L"], ref[0]["R"], True)


# ---- 1. full batches
@pytest.mark.parametrize("F", [2, 4])
def test_full_batches(refs, F):
    """groups of 4 on 8 engines, three groups back to back: every front launch carries F members"""
    r = [refs(k) for k in range(12)]
    ctx = _context(8, 4, F)
    try:
        for k in range(12):
            _put(ctx, 2 + k, r[k])
        assert _closed(ctx) == (3, 0, 0, 0, 0)
        assert _cost_entries(ctx) == [F] * (12 // F)
        for k in range(12):
            _check(ctx, 2 + (k * 5) % 12, r[(k * 5) % 12], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 2. partial flushes
@pytest.mark.parametrize("how", ["consumer", "flush", "synchronize"])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_partial_flushes(refs, n, how):
    """F = 3, groups of 6: the group closes with n members submitted -- 1, F - 1 or 1 (behind one full batch) front pending -- by a
    consumer of a member's slot, by vo_lookahead_flush, or by vo_synchronize; further submissions follow and open a group of
    their own"""
    r = [refs(k) for k in range(n + 2)]
    ctx = _context(8, 6, 3)
    try:
        for k in range(n):
            _put(ctx, 2 + k, r[k])
        first = [3, 1] if n == 4 else [n]
        assert _cost_entries(ctx) == first[:-1]
        assert _closed(ctx) == (0, 0, 0, 0, n)
        if how == "consumer":
            _check(ctx, 2, r[0], "the member that closes")
            assert _closed(ctx) == (0, 1, 0, 0, 0)
        elif how == "flush":
            ctx.lookahead_flush()
            assert _closed(ctx) == (0, 0, 1, 0, 0)
        else:
            ctx.synchronize()
            assert _closed(ctx) == (0, 1, 0, 0, 0)
        assert _cost_entries(ctx) == first
        for k in (n, n + 1):
            _put(ctx, 2 + k, r[k])
        assert ctx.sweep_group_stats()["open"] == 2
        assert _cost_entries(ctx) == first
        ctx.lookahead_flush()
        assert _cost_entries(ctx) == first + [2]
        for k in range(n + 2):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 3. mixed sources in one batch
def test_mixed_sources_in_one_batch(oracle, refs):
    """one batch of 5: a staged pair read in place, a pair out of the pinned staging buffers, a pair from host memory, a staged
    pair that is not preprocessed (remapped on its way in: no in-place ingest) and a host pair that is not preprocessed"""
    r = [refs(k) for k in range(5)]
    ys, xs = np.mgrid[0:H, 0:W]
    map1, map2 = np.stack([xs, ys], 2).astype(np.int16), np.zeros((H, W), np.uint16)
    for k in (3, 4):
        for side in ("L", "R"):
            assert np.array_equal(oracle.remap_bilinear(r[k][0][side], map1, map2), r[k][0][side])    # the identity: refs(k) holds
    ctx = _context(8, 5, 5)
    try:
        ctx.set_rectify_maps(0, map1, map2)
        ctx.set_rectify_maps(1, map1, map2)
        ctx.stage_pairs([(r[k][0]["L"], r[k][0]["R"]) for k in range(5)])
        ctx.host_stage_pair(1, r[1][0]["L"], r[1][0]["R"])
        ctx.prefetch_staged_pair(2, 0, True)
        ctx.prefetch_host_staged(3, 1, W, H, 1, True)
        _put(ctx, 4, r[2])
        ctx.prefetch_staged_pair(5, 3, False)
        assert _cost_entries(ctx) == []
        ctx.prefetch_pair(6, r[4][0]["L"], r[4][0]["R"], False)
        assert _closed(ctx) == (1, 0, 0, 0, 0)
        assert _cost_entries(ctx) == [5]
        for k in range(5):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 4. source lifetime
@pytest.mark.parametrize("what", ["reallocate", "overwrite"])
def test_staged_sources_change_with_fronts_pending(refs, what):
    """two staged pairs submitted in place, their fronts pending; then the staged pairs are allocated anew, or one of them is
    overwritten.  The results are those of the images submitted."""
    r = [refs(k) for k in range(4)]
    ctx = _context(8, 4, 4)
    try:
        ctx.stage_pairs([(r[k][0]["L"], r[k][0]["R"]) for k in (0, 1)])
        ctx.prefetch_staged_pair(2, 0, True)
        ctx.prefetch_staged_pair(3, 1, True)
        assert _closed(ctx) == (0, 0, 0, 0, 2) and _cost_entries(ctx) == []
        if what == "reallocate":
            ctx.stage_pairs([(r[k][0]["L"], r[k][0]["R"]) for k in (2, 3, 0)])
        else:
            L, R = (_native._c(r[2][0][s], np.uint8) for s in ("L", "R"))
            ctx._ck(ctx._lib.vo_stage_pair(ctx._h, 0, _native._p(L), _native._p(R)))
        assert _cost_entries(ctx) == [2]                          # launched before the images went
        assert ctx.sweep_group_stats()["open"] == 2               # ... and the group goes on
        ctx.prefetch_staged_pair(4, 0, True)                      # pair 2, either way
        _put(ctx, 5, r[3])
        assert _closed(ctx) == (1, 0, 0, 0, 0)
        assert _cost_entries(ctx) == [2, 2]
        for k in range(4):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 5. parameters
def test_parameters_change_between_submissions(refs):
    """vo_set_sgbm with another P2 and block size between two submissions: every pair is exact for the parameters in force at
    its own submission"""
    q = params(D, P2=1200, blockSize=3)
    r = [refs(0), refs(1), refs(2, q), refs(3, q), refs(4)]
    ctx = _context(8, 4, 4)
    try:
        _put(ctx, 2, r[0])
        _put(ctx, 3, r[1])
        ctx.set_sgbm(q)
        assert _closed(ctx) == (0, 0, 0, 1, 0) and _cost_entries(ctx) == [2]
        _put(ctx, 4, r[2])
        _put(ctx, 5, r[3])
        ctx.set_sgbm(P)
        assert _closed(ctx) == (0, 0, 0, 2, 0) and _cost_entries(ctx) == [2, 2]
        _put(ctx, 6, r[4])
        for k in reversed(range(5)):
            _check(ctx, 2 + k, r[k], k)
        assert _cost_entries(ctx) == [2, 2, 1]
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 6. runs that do not defer their front
@pytest.mark.parametrize("kind", ["mode_hh", "uniqueness_100", "nothing_to_compute", "odd_width"])
def test_runs_that_do_not_defer_between_deferring_pairs(oracle, refs, kind):
    """F = 3, groups of 3 on 4 engines: a run that launches its own front -- entries 1 -- between pairs that leave theirs to the
    group.  MODE_HH and uniquenessRatio 100 never defer (the setter closes the open group); W1 <= 0 has nothing to compute and
    no front at all; W1 % 16 != 0 is not k_sgbm_we2's geometry: the run joins a group of its own behind its own front."""
    r = [refs(k) for k in range(5)]
    ctx = _context(4, 3, 3)
    try:
        _put(ctx, 2, r[0])
        assert ctx.sweep_group_stats()["open"] == 1 and _cost_entries(ctx) == []
        if kind == "nothing_to_compute":
            L, R = pair(D, H, 40, D, 0)
            odd = oracle.sgbm_compute(L, R, P, 0)
            ctx.prefetch_pair(9, L, R, True)
            assert _closed(ctx) == (0, 0, 0, 0, 1) and _cost_entries(ctx) == []
            want = [3, 2]
        elif kind == "odd_width":
            assert (216 - D) % 16 != 0
            odd = refs(7, P, 0, 216)
            _put(ctx, 9, odd)
            assert _closed(ctx) == (0, 0, 0, 1, 1) and _cost_entries(ctx) == [1, 1]     # its own front, then the closing group's
            want = [1, 1, 3, 1]
        else:
            p, mode = (P, 1) if kind == "mode_hh" else (params(D, uniquenessRatio=100), 0)
            odd = refs(7, p, mode)
            ctx.set_sgbm(p, mode)
            assert _closed(ctx) == (0, 0, 0, 1, 0) and _cost_entries(ctx) == [1]
            _put(ctx, 9, odd)
            assert ctx.sweep_group_stats()["open"] == 0 and _cost_entries(ctx) == [1, 1]
            ctx.set_sgbm(P)
            want = [1, 1, 3, 1]
        for k in (1, 2, 3, 4):
            _put(ctx, 2 + k, r[k])
        if kind == "nothing_to_compute":
            got = disp16(ctx, 9, D, H)
            assert np.array_equal(got, odd) and (got < 0).all()
        else:
            _check(ctx, 9, odd, kind, 216 if kind == "odd_width" else W)
        for k in range(5):
            _check(ctx, 2 + k, r[k], k)
        assert _cost_entries(ctx) == want
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


# ---- 7. kernel variants through a batch of 3
VARIANTS = {
    "block1": (W, params(D, blockSize=1)),                       # ring in registers
    "block3": (W, params(D, blockSize=3)),
    "block5": (W, P),
    "block7": (W, params(D, blockSize=7)),                       # ring in LDS
    "block11": (W, params(D, blockSize=11)),                     # the largest block vo_set_sgbm takes
    "D48": (W, params(48)),                                      # padded to 64
    "D160": (WMAX, params(160)),                                 # two waves per workgroup
    "minD-8": (W, params(D, minD=-8)),
    "minD+16": (W, params(D, minD=16)),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_kernel_variants_through_a_batch(refs, name):
    w, p = VARIANTS[name]
    minX1 = max(p["minDisparity"] + p["numDisparities"], 0)
    W1 = w + min(p["minDisparity"], 0) - minX1
    assert W1 % 16 == 0 and W1 >= 32, (name, W1)                 # the runs defer
    assert min(strip_kinds(w, p)) >= 1                           # both paths of the cost sweep
    r = [refs(k, p, 0, w) for k in range(3)]
    ctx = _context(4, 3, 3, p, w, p["numDisparities"])
    try:
        for k in range(3):
            _put(ctx, 2 + k, r[k])
        assert _closed(ctx) == (1, 0, 0, 0, 0)
        assert _cost_entries(ctx) == [3]
        for k in range(3):
            _check(ctx, 2 + k, r[k], (name, k), w)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_block_13_is_refused():
    ctx = _context(4, 3, 3)
    try:
        with pytest.raises(_native.VoError):
            ctx.set_sgbm(params(D, blockSize=13))
    finally:
        ctx.close()


# ---- 8. drop with fronts pending; a submission that fails
def test_drop_with_fronts_pending_then_a_fresh_group(refs):
    r = [refs(k) for k in range(6)]
    ctx = _context(8, 4, 4)
    try:
        _put(ctx, 2, r[0])
        _put(ctx, 3, r[1])
        assert _closed(ctx) == (0, 0, 0, 0, 2) and _cost_entries(ctx) == []
        ctx.lookahead_drop(2)
        assert _closed(ctx) == (0, 1, 0, 0, 0) and _cost_entries(ctx) == [2]
        for k in range(2, 6):
            _put(ctx, 2 + k, r[k])
        assert _closed(ctx) == (1, 1, 0, 0, 0) and _cost_entries(ctx) == [2, 4]
        for k in range(6):
            _check(ctx, 2 + k, r[k], k)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def _failed_submission_body(out):
    """Body of test_failed_submission_with_fronts_pending: a process of its own against the test-only build of the library.
    VO_FAULT_PREFETCH=3 makes the third look-ahead submission return a status inside its engine scope: a status, not a fault."""
    pairs = [pair(W, H, k, D, 0) for k in range(5)]
    os.environ["VO_FAULT_PREFETCH"] = "3"
    ctx = _context(8, 4, 4)
    del os.environ["VO_FAULT_PREFETCH"]
    res = {}
    try:
        ctx.prefetch_pair(2, *pairs[0], True)
        ctx.prefetch_pair(3, *pairs[1], True)
        with pytest.raises(_native.VoError):
            ctx.prefetch_pair(4, *pairs[2], True)
        assert _closed(ctx) == (0, 0, 0, 0, 2) and _cost_entries(ctx) == []
        ctx.prefetch_pair(5, *pairs[3], True)
        ctx.prefetch_pair(6, *pairs[4], True)
        assert _closed(ctx) == (1, 0, 0, 0, 0) and _cost_entries(ctx) == [4]
        with pytest.raises(_native.VoError):                      # the failed slot hands nothing out
            ctx.download_disparity_f32(4, (H, W))
        for k in (0, 1, 3, 4):
            res["disp%d" % k] = disp16(ctx, 2 + k, W, H)
            for name, v in _keypoints(ctx, 2 + k).items():
                res["%s%d" % (name, k)] = np.ascontiguousarray(v)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()
    np.savez(out, **res)
    print("failed-submission body ok")


def test_failed_submission_with_fronts_pending(tmp_path, refs):
    hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
    assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
    out = str(tmp_path / "failed.npz")
    code = "import tests.test_gpu_group_fronts as t; t._failed_submission_body(%r)" % out
    child = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=300)
    assert child.returncode == 0 and "failed-submission body ok" in child.stdout, child.stdout[-2000:] + child.stderr[-4000:]
    got = np.load(out)
    for k in (0, 1, 3, 4):
        c, kp, (kp1, d1) = refs(k)
        assert np.array_equal(got["disp%d" % k], c["ref"]) and np.array_equal(d1, c["ref"]), k
        _same({name: got["%s%d" % (name, k)] for name in FIELDS}, kp, ("oracle", k))
        _same({name: got["%s%d" % (name, k)] for name in FIELDS}, kp1, ("alone", k))


# ---- 9. the off switch
def _payload():
    """what the off-switch test compares: three groups of 4 on 8 engines under the environment's VO_GROUP_FRONTS (unset: the
    default), disparities and keypoints of all twelve pairs and the entries of the sgbm_cost brackets"""
    ctx = _native.Context(0, W, H, D, NF, engines=8)
    try:
        ctx.set_sgbm(P)
        ctx.lookahead_orb(*ORB)
        assert ctx.set_sweep_group(4) == 4
        ctx.enable_timing(True)
        for k in range(12):
            ctx.prefetch_pair(2 + k, *pair(W, H, k, D, 0), True)
        assert _closed(ctx) == (3, 0, 0, 0, 0)
        out = {"cost_entries": np.array(_cost_entries(ctx), np.int32)}
        for k in range(12):
            out["disp%d" % k] = disp16(ctx, 2 + k, W, H)
            for name, v in _keypoints(ctx, 2 + k).items():
                out["%s%d" % (name, k)] = np.ascontiguousarray(v)
        assert ctx.sgbm_sweep_status() == 0
        return out
    finally:
        ctx.close()


def test_off_switch(tmp_path, refs):
    """VO_GROUP_FRONTS=0 in a fresh process: every run launches its own front, and every byte is the same"""
    here = _payload()
    assert here["cost_entries"].tolist() == [4, 4, 4]            # the default batch is a whole group of 4
    for k in range(12):
        assert np.array_equal(here["disp%d" % k], refs(k)[0]["ref"]), k
    out = str(tmp_path / "off.npz")
    child = subprocess.run([sys.executable, "-m", "tests.test_gpu_group_fronts", out], cwd=ROOT, env=dict(os.environ, VO_GROUP_FRONTS="0"),
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    off = np.load(out)
    assert sorted(off.files) == sorted(here)
    assert off["cost_entries"].tolist() == [1] * 12
    for name in here:
        if name != "cost_entries":
            assert here[name].shape == off[name].shape and np.array_equal(here[name].view(np.uint8), off[name].view(np.uint8)), name


if __name__ == "__main__":
    np.savez(sys.argv[1], **_payload())
