"""The ORB chain of a sweep group's members runs as ONE launch per kernel (k_orb_pyramid, k_orb_fast_nms, k_orb_select,
k_orb_describe) on the closing member's stream, the member picked by a block index out of a table in the kernel arguments; no
other member's stream receives anything at close, an engine orders itself behind the chain when it is next given work.
Whatever group a pair travels in, its keypoints (xy, angle, octave, response, size) and descriptors equal the oracle's ORB on
the mask of the oracle's own disparity, and those of the same pair streamed at group size 1 into another slot, bit for bit;
its disparity equals both as group_inputs.check() has it.  Every member of a group gets a different pair, and every case shows
on the oracle alone that its input loads the batched launches.  Every case starts on a fresh context: no slot, engine or
workspace holds an earlier answer that a chain started too early, or never, could pass off as its own."""
import numpy as np
import pytest

from openvo_amd import _native
from tests.group_inputs import Coverage, disp16, pair, params

pytestmark = pytest.mark.gpu

FIELDS = ("xy", "angle", "octave", "response", "size", "desc")
MASK = (16, 640)                                                        # the fused mask keeps disparities of 1 .. 40 pixels
GROUP0, ALONE0 = 2, 15                                                  # first slot of the run under test / of the run at group size 1


@pytest.fixture(scope="module")
def cov(oracle):
    return Coverage(oracle)


@pytest.fixture(scope="module")
def orb_ref(oracle):
    """oracle keypoints of (left image, oracle disparity) under a request, once per input and never changed afterwards"""
    memo = {}

    def get(key, L, ref, nfeatures, mask_mode=1, roi=None):
        key = (key, nfeatures, mask_mode, roi)
        if key not in memo:
            mask = ((ref >= MASK[0]) & (ref <= MASK[1])).astype(np.uint8) * 255 if mask_mode else None
            if roi is not None:
                x0, y0, x1, y1 = roi
                L = L[y0:y1, x0:x1]
                mask = mask[y0:y1, x0:x1] if mask is not None else None
            k = oracle.orb_detect_and_compute(L, mask, nfeatures, cap=2 * nfeatures + 8192)
            for v in k.values():
                v.setflags(write=False)
            memo[key] = k
        return memo[key]
    return get


def _request(nfeatures, mask_mode=1):
    return (nfeatures, mask_mode, MASK[0], MASK[1]) if mask_mode else (nfeatures, 0, 0, 0)


def _submit(ctx, members, B, slot0, order=None):
    assert ctx.set_sweep_group(B) == B
    for i in (order if order is not None else range(len(members))):
        ctx.prefetch_pair(slot0 + i, members[i]["L"], members[i]["R"], True)


def _read(ctx, slot, request, w, h):
    k = ctx.orb_slot(slot, *request)
    return {name: v.copy() for name, v in k.items()}, disp16(ctx, slot, w, h)


def _same(a, b, what):
    for name in FIELDS:
        assert a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint8), np.ascontiguousarray(b[name]).view(np.uint8)), (what, name)


def _exact(group, alone, m, ref_kp, what):
    """a member's result in the group and alone against the oracle, all three ways (disparities as group_inputs.check)"""
    (kg, dg), (ka, da) = group, alone
    assert np.array_equal(da, m["ref"]), (what, "disparity alone vs oracle", int((da != m["ref"]).sum()))
    assert np.array_equal(dg, m["ref"]), (what, "disparity group vs oracle", int((dg != m["ref"]).sum()))
    assert np.array_equal(dg, da), (what, "disparity group vs alone")
    _same(ka, ref_kp, (what, "alone vs oracle"))
    _same(kg, ref_kp, (what, "group vs oracle"))
    _same(kg, ka, (what, "group vs alone"))


def _group_then_alone(ctx, members, B, request, w, h, order=None):
    """the members in groups of B into slots GROUP0.., read in another order than submitted; then the same pairs at group size 1
    into slots ALONE0.., each on another engine than before"""
    n = len(members)
    _submit(ctx, members, B, GROUP0, order)
    got = [_read(ctx, GROUP0 + i, request, w, h) for i in reversed(range(n))][::-1]
    _submit(ctx, members, 1, ALONE0, [(i + 1) % n for i in range(n)])
    assert ctx.sweep_group_stats()["open"] == 0
    alone = [_read(ctx, ALONE0 + i, request, w, h) for i in range(n)]
    return got, alone


def _levels(k):
    return sorted(set(int(o) for o in k["octave"]))


@pytest.mark.parametrize("B", [1, 2, 5, 12])
def test_member_indexing(cov, orb_ref, B):
    """224 x 96, D = 64, 300 features: a different pair per member -- a swapped table entry cannot pass.  On the oracle: every
    member has at least 100 keypoints on levels 0, 1 and 2 (measured 137-146), no two members the same descriptors."""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    members = cov.group(w, h, list(range(B)), p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    for r in refs:
        assert len(r["xy"]) >= 100 and set(_levels(r)) >= {0, 1, 2}, (len(r["xy"]), _levels(r))
    assert len(set(r["desc"].tobytes() for r in refs)) == B
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, B, _request(nf), w, h)
        st = ctx.sweep_group_stats()
        assert (st["full"], st["consumer"], st["flush"], st["other"], st["open"]) == (1 if B > 1 else 0, 0, 0, 0, 0)
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], (B, i))
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_quotas_cut_below_capacity(cov, orb_ref):
    """40 features in a group of 12: the per-level quotas -- one level table for all members -- decide, not a list's capacity
    (the oracle keeps 22 per member of more than 500 candidates)"""
    w, h, D, nf = 224, 96, 64, 40
    p = params(D)
    members = cov.group(w, h, list(range(12)), p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    for k, (m, r) in enumerate(zip(members, refs)):
        uncapped = orb_ref((w, h, k, D), m["L"], m["ref"], 5000)
        assert 0 < len(r["xy"]) < len(uncapped["xy"]), (k, len(r["xy"]), len(uncapped["xy"]))
    ctx = _native.Context(0, w, h, D, 300)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, 12, _request(nf), w, h)
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_more_pyramid_levels(cov, orb_ref):
    """320 x 160, D = 32: keypoints on six levels and more (the oracle gives 234-236 per member on levels 0-5), a group of 12"""
    w, h, D, nf = 320, 160, 32, 300
    p = params(D)
    members = cov.group(w, h, list(range(12)), p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    for r in refs:
        assert len(_levels(r)) >= 6 and len(r["xy"]) >= 200, (_levels(r), len(r["xy"]))
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, 12, _request(nf), w, h)
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_member_with_nothing(oracle, cov, orb_ref, where):
    """two constant images as the first, the middle and the last (closing) member of a group of 3: the oracle finds no
    disparity inside the mask's range and no keypoint for it; the other members are exact and the empty one's count is 0"""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    flat = np.full((h, w), 128, np.uint8)
    flat_ref = oracle.sgbm_compute(flat, flat, p, 0)
    assert not ((flat_ref >= MASK[0]) & (flat_ref <= MASK[1])).any()     # no pixel the fused mask lets through
    empty = dict(L=flat, R=flat, ref=flat_ref)
    real = cov.group(w, h, [0, 1], p)
    members = real[:where] + [empty] + real[where:]
    real_keys = [(w, h, 0, D), (w, h, 1, D)]
    keys = real_keys[:where] + [("flat", w, h, D)] + real_keys[where:]
    refs = [orb_ref(key, m["L"], m["ref"], nf) for key, m in zip(keys, members)]
    assert [len(r["xy"]) == 0 for r in refs] == [i == where for i in range(3)]
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, 3, _request(nf), w, h)
        assert ctx.sweep_group_stats()["full"] == 1
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], (where, i))
        assert len(got[where][0]["xy"]) == 0
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_no_mask(cov, orb_ref):
    """mask_mode 0 in a group of 3: the pyramid kernel's instance without the mask"""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    members = cov.group(w, h, [3, 4, 5], p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf, 0) for k, m in zip((3, 4, 5), members)]
    masked = [orb_ref((w, h, k, D), m["L"], m["ref"], nf, 1) for k, m in zip((3, 4, 5), members)]
    for r, q in zip(refs, masked):
        assert len(r["xy"]) >= 100 and r["desc"].tobytes() != q["desc"].tobytes()      # (the mask would have mattered)
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf, 0))
        got, alone = _group_then_alone(ctx, members, 3, _request(nf, 0), w, h)
        assert ctx.sweep_group_stats()["full"] == 1
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
    finally:
        ctx.close()


def test_roi_cropping_all_four_sides(cov, orb_ref):
    """a ROI set before the group: every member's source pointers start inside its image, the strides stay the image's"""
    w, h, D, nf = 224, 96, 64, 300
    roi = (9, 5, 215, 90)
    p = params(D)
    members = cov.group(w, h, [6, 7, 8], p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf, 1, roi) for k, m in zip((6, 7, 8), members)]
    whole = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in zip((6, 7, 8), members)]
    for r, q in zip(refs, whole):
        assert len(r["xy"]) >= 50 and r["desc"].tobytes() != q["desc"].tobytes()       # (the crop matters)
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.set_roi(*roi)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, 3, _request(nf), w, h)
        assert ctx.sweep_group_stats()["full"] == 1
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
    finally:
        ctx.close()


def test_engine_0_member_closing_and_not_with_a_synchronous_run_behind_each_group(oracle, cov, orb_ref):
    """engine 0's member works in the main SGBM workspace and in the ORB scratch of engine 0: as a non-closing member
    (engines 0, 1) and as the closing one (engines 2, 0), a synchronous run in the main workspace directly behind each group"""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    members = cov.group(w, h, [0, 1, 2, 3], p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    sync = [pair(w, h, 10), pair(w, h, 11)]
    sync_ref = [oracle.sgbm_compute(L, R, p, 0) for (L, R) in sync]
    ctx = _native.Context(0, w, h, D, nf, engines=3)                   # a fresh context: its first pair goes to engine 0
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        _submit(ctx, members[:2], 2, GROUP0)                           # engines 0, 1: engine 1 closes
        assert ctx.sweep_group_stats()["open"] == 0
        got_sync0 = ctx.sgbm_compute_host(*sync[0])
        _submit(ctx, members[2:], 2, GROUP0 + 2)                       # engines 2, 0: engine 0 closes
        assert ctx.sweep_group_stats()["open"] == 0
        got_sync1 = ctx.sgbm_compute_host(*sync[1])
        assert ctx.sweep_group_stats()["full"] == 2
        assert np.array_equal(got_sync0, sync_ref[0]) and np.array_equal(got_sync1, sync_ref[1])
        got = [_read(ctx, GROUP0 + i, _request(nf), w, h) for i in range(4)]
        _submit(ctx, members, 1, ALONE0, [1, 2, 3, 0])
        alone = [_read(ctx, ALONE0 + i, _request(nf), w, h) for i in range(4)]
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_lazy_ordering_of_engines_between_groups(cov, orb_ref):
    """three engines, two groups of 3 back to back on the same engines with six different pairs and no host wait between the
    submissions: the second group's fronts reuse the workspaces and the ORB scratch the first group's chain -- on ONE of
    their streams -- is still working in, and nothing but the wait an engine takes when it is next given work orders them.  A
    third round at group size 1 runs on those engines as well."""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    members = cov.group(w, h, list(range(9)), p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    ctx = _native.Context(0, w, h, D, nf, engines=3)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        assert ctx.set_sweep_group(3) == 3
        for i in range(6):
            ctx.prefetch_pair(GROUP0 + i, members[i]["L"], members[i]["R"], True)
        assert ctx.sweep_group_stats()["full"] == 2
        assert ctx.set_sweep_group(1) == 1
        for i in range(6, 9):
            ctx.prefetch_pair(GROUP0 + i, members[i]["L"], members[i]["R"], True)
        got = [_read(ctx, GROUP0 + i, _request(nf), w, h) for i in range(9)]
        _submit(ctx, members, 1, ALONE0, [(i + 1) % 9 for i in range(9)])
        alone = [_read(ctx, ALONE0 + i, _request(nf), w, h) for i in range(9)]
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_groups_closed_by_a_consumer_by_a_flush_and_by_a_geometry_change(cov, orb_ref):
    w, h, D, nf = 224, 96, 64, 300
    w2 = 240                                                            # W1 = 176: k_sgbm_we2 as well, another geometry
    p = params(D)
    rq = _request(nf)
    jobs = [(w, 0), (w, 1), (w, 2), (w, 3), (w, 4), (w, 5), (w, 6), (w2, 0), (w2, 1)]
    members = [cov.get(jw, h, k, p) for (jw, k) in jobs]
    refs = [orb_ref((jw, h, k, D), m["L"], m["ref"], nf) for (jw, k), m in zip(jobs, members)]
    ctx = _native.Context(0, w2, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*rq)
        assert ctx.set_sweep_group(4) == 4
        got = [None] * len(jobs)
        # a consumer: the keypoints of the first member with two of four members open
        s0 = ctx.sweep_group_stats()
        for i in (0, 1):
            ctx.prefetch_pair(GROUP0 + i, members[i]["L"], members[i]["R"], True)
        assert ctx.sweep_group_stats()["open"] == 2
        k0 = ctx.orb_slot(GROUP0, *rq)
        s1 = ctx.sweep_group_stats()
        assert s1["consumer"] - s0["consumer"] == 1 and s1["open"] == 0
        got[0] = ({name: v.copy() for name, v in k0.items()}, disp16(ctx, GROUP0, w, h))
        got[1] = _read(ctx, GROUP0 + 1, rq, w, h)
        # a flush with three of four
        for i in (2, 3, 4):
            ctx.prefetch_pair(GROUP0 + i, members[i]["L"], members[i]["R"], True)
        assert ctx.sweep_group_stats()["open"] == 3
        ctx.lookahead_flush()
        s2 = ctx.sweep_group_stats()
        assert s2["flush"] - s1["flush"] == 1 and s2["open"] == 0
        # the geometry changes in mid-stream: the third submission closes the first group
        for n, i in enumerate((5, 6, 7, 8)):
            ctx.prefetch_pair(GROUP0 + i, members[i]["L"], members[i]["R"], True)
            assert ctx.sweep_group_stats()["open"] == (1, 2, 1, 2)[n]
        s3 = ctx.sweep_group_stats()
        assert s3["other"] - s2["other"] == 1 and s3["full"] == s2["full"]
        ctx.lookahead_flush()
        for i in range(2, 9):
            got[i] = _read(ctx, GROUP0 + i, rq, jobs[i][0], h)
        _submit(ctx, members, 1, ALONE0, [(i + 1) % 9 for i in range(9)])
        alone = [_read(ctx, ALONE0 + i, rq, jobs[i][0], h) for i in range(9)]
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
        assert ctx.sgbm_sweep_status() == 0
    finally:
        ctx.close()


def test_more_than_2000_features(cov, orb_ref):
    """nfeatures 2500 takes the three-launch selection, which stays one member per launch -- on the closing member's stream
    like the rest of the chain.  The oracle finds about 3900 candidates per member: the quotas bind."""
    w, h, D, nf = 320, 160, 32, 2500
    p = params(D)
    members = cov.group(w, h, [0, 1], p)
    refs = [orb_ref((w, h, k, D), m["L"], m["ref"], nf) for k, m in enumerate(members)]
    for k, (m, r) in enumerate(zip(members, refs)):
        uncapped = orb_ref((w, h, k, D), m["L"], m["ref"], 20000)
        assert 0 < len(r["xy"]) < len(uncapped["xy"]), (k, len(r["xy"]), len(uncapped["xy"]))
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        got, alone = _group_then_alone(ctx, members, 2, _request(nf), w, h)
        assert ctx.sweep_group_stats()["full"] == 1
        for i, m in enumerate(members):
            _exact(got[i], alone[i], m, refs[i], i)
    finally:
        ctx.close()


def test_stage_timer_counts_members(cov):
    """with timing on, the ORB bracket of a group of 5 counts 5 and a positive time: timings()["orb"] stays a per-pair figure"""
    w, h, D, nf = 224, 96, 64, 300
    p = params(D)
    members = cov.group(w, h, [0, 1, 2, 3, 4], p)
    ctx = _native.Context(0, w, h, D, nf)
    try:
        ctx.set_sgbm(p)
        ctx.lookahead_orb(*_request(nf))
        ctx.enable_timing(True)
        before = ctx.timings()["orb"]
        _submit(ctx, members, 5, GROUP0)
        assert ctx.sweep_group_stats()["full"] == 1
        counts = [len(ctx.orb_slot(GROUP0 + i, *_request(nf))["xy"]) for i in range(5)]
        assert min(counts) >= 100
        ctx.synchronize()
        after = ctx.timings()["orb"]
        assert after[1] - before[1] == 5 and after[0] > before[0], (before, after)
    finally:
        ctx.close()
