"""tests/planted_mono.py and tests/mono_pose_ref.py held to independent references on the CPU, so that a failure of
tests/test_gpu_planted_mono.py points at the kernel: the planted votes against the requested counts, the restated decomposition
against LAPACK, the lower median against numpy.sort, the flags of a zero / non-finite E, and that every regime the GPU module
promises is reached by its cases."""
import numpy as np
import pytest

import mono_pose_ref as ref
import planted_mono as PM


def test_planted_votes_equal_the_requested_counts():
    arms, winners = set(), set()
    for e, (name, E) in enumerate(PM.vote_essentials()):
        tr1, tr2 = PM.traces(E)
        R1, R2, t = ref.decompose(E)
        for c, counts4 in enumerate(PM.VOTE_COUNTS):
            p1, p2 = PM.vote_scene(E, counts4, 100 * e + c)
            cls, safe = PM.classes(E, p1, p2)
            assert safe.all() and np.abs(p1).max() <= PM.PIX_MAX and np.abs(p2).max() <= PM.PIX_MAX
            # counted one pair at a time, without ref.vote: each pair votes for at most one candidate
            assert [int((cls == k).sum()) for k in range(4)] == list(counts4) and ((cls >= -1) & (cls <= 3)).all()
            votes4, winner = ref.vote(R1, R2, t, ref.normalise(p1, PM.K4), ref.normalise(p2, PM.K4), np.ones(len(p1), bool))
            assert list(votes4) == list(counts4), (name, counts4)
            arms |= PM.tie_arms(counts4, tr1, tr2)
            winners.add(winner)
    assert {tr[0] > tr[1] for tr in (PM.traces(E) for _, E in PM.vote_essentials())} == {True, False}
    assert arms == PM.ALL_TIE_ARMS and winners == {0, 1, 2, 3}
    p1, p2 = PM.stride_scene(1025)
    assert len(p1) == 1025


def test_restated_decomposition_against_lapack():
    seen = set()
    for name, E, kind in PM.essentials():
        if kind == "refused":
            continue
        R1, R2, t = ref.decompose(E)
        U, w, _ = np.linalg.svd(E)
        for R in (R1, R2):
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12, name
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12
        if kind == "full":
            assert w[1] > 0 and min(np.abs(t - U[:, 2]).max(), np.abs(t + U[:, 2]).max()) <= 1e-12, name
        else:
            assert w[1] <= 1e-300 and abs(t @ U[:, 0]) <= 1e-12, name
        # the arms of svd3 this entry takes
        _, sv, _ = ref.svd3(E)
        tiny = sv[0] * 1e-300 + 1e-300
        seen.add(("w1", bool(sv[1] <= tiny)))
        seen.add(("w2", bool(sv[2] <= tiny or sv[2] <= 1e-14 * sv[0])))
        if name.startswith("rank1"):
            seen.add(("a", bool(abs(E[:, np.argmax(np.abs(E).sum(0))][0] / sv[0]) > 0.9)))
        if name.startswith("order_"):
            norms = np.linalg.norm(E, axis=0)
            seen.add(("order", tuple(int(k) for k in np.argsort(-norms, kind="stable"))))
    assert {s for s in seen if s[0] != "order"} == {("w1", True), ("w1", False), ("w2", True), ("w2", False), ("a", True), ("a", False)}
    assert {s[1] for s in seen if s[0] == "order"} == set(PM.PERMS)          # every outcome of the three-compare sort
    # the ladder crosses the 1e-14 threshold between its third and fourth step
    sv = {name: ref.svd3(E)[1] for name, E, _ in PM.essentials() if name.startswith("ladder_")}
    assert sv["ladder_1e-15"][2] <= 1e-14 * sv["ladder_1e-15"][0] and sv["ladder_2e-14"][2] > 1e-14 * sv["ladder_2e-14"][0]


def test_flags_of_a_zero_or_non_finite_essential():
    p1, p2 = PM.vote_scene(PM.essential(1), (5, 0, 0, 0), 7)
    for name, E, kind in PM.essentials():
        r = ref.recover_pose(E, p1, p2, PM.K4, depth_a=np.ones(5))
        assert (r["flags"] == 1) == (kind == "refused"), name
        if kind == "refused":
            assert np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and not r["votes4"].any() and not r["z1"].any()
    assert ref.recover_pose(PM.essential(1), p1, p2, PM.K4)["flags"] == 4
    assert ref.recover_pose(np.zeros((3, 3)), p1, p2, PM.K4)["flags"] == 5


@pytest.mark.parametrize("case", PM.SELECT_CASES)
def test_lower_median_against_sort(case):
    z1 = np.random.default_rng(3).uniform(0.4, 20.0, PM.SELECT_N)
    d, shared = PM.select_depths(case, z1)
    ratios, sh = PM.actual_ratios(d, z1)
    assert np.array_equal(sh, shared) and len(ratios) == int(shared.sum())
    got = ref.lower_median(ratios)
    s = np.sort(ratios)
    k = (len(s) - 1) // 2
    assert got == s[k] and (s <= got).sum() >= k + 1 and (s < got).sum() <= k
    pat = ratios.view(np.uint64)
    assert (pat != np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    # each case is the regime its name promises
    if case == "all_equal":
        assert len(set(pat)) == 1
    elif case.startswith("split"):
        lo = int(case.split("_")[1])
        assert (ratios == 0.5).sum() == lo and (ratios == 2.0).sum() == PM.SELECT_N - lo and got == (0.5 if lo > k else 2.0)
        assert {int(p) >> 56 for p in pat} == {0x3F, 0x40}                  # bins 63 | 64: the last of one scan lane, the first of the next
    elif case == "low_bytes":
        off = pat.astype(np.int64) - np.int64(PM.LOW_BYTES_START)
        assert off.min() >= -2 and off.max() <= PM.SELECT_N + 2 and len(set(pat)) > PM.SELECT_N // 2
        assert (ratios < 1.0).any() and (ratios >= 1.0).any()
    elif case == "top_bytes":
        assert not (pat & np.uint64((1 << 52) - 1)).any() and len({int(p) >> 56 for p in pat}) > 40
    elif case == "run_300":
        assert (ratios == 1.0).sum() == 300 and (ratios < 1.0).sum() <= k < (ratios <= 1.0).sum() and got == 1.0
    elif case == "extremes":
        assert (ratios == 0.0).any() and np.isinf(ratios).any() and got > 1e300
    else:
        assert len(ratios) == int(case.split("_")[1])


def test_planted_parallax_sits_where_it_was_asked():
    s = PM.gate_scene()
    sin2 = PM.sin2_of(s["R"], s["t"], s["p1"], s["p2"])
    assert len(sin2) == 64 and (sin2[56:60] > PM.GATE).all() and (sin2[60:] < PM.GATE).all()
    assert (np.abs(sin2[56:] / PM.GATE - 1.0) < 1e-9).all() and (np.abs(sin2[:56] / PM.GATE - 1.0) > 0.009).all()
    cls, safe = PM.classes(s["E"], s["p1"], s["p2"])
    assert safe.all() and len(set(cls)) == 1 and cls[0] in (0, 1, 2, 3)    # all 64 vote for the planted pose
    r = ref.recover_pose(s["E"], s["p1"], s["p2"], PM.K4, gate=PM.GATE)
    assert np.abs(r["R"] - s["R"]).max() <= 1e-12 and np.abs(r["t"] - s["t"]).max() <= 1e-12
    want = np.r_[sin2[:56] > PM.GATE, [True] * 4, [False] * 4]
    assert np.array_equal(r["valid"], want) and r["n_depth"] == int(want.sum())


def test_finish_frames_leave_the_promised_matches(oracle):
    for name, (seed, M) in PM.FINISH_SEEDS.items():
        a, b = PM.finish_frames(seed)
        ka, kb = oracle.orb_detect_and_compute(a, None, 2000), oracle.orb_detect_and_compute(b, None, 2000)
        idx, dist = oracle.bf_knn2_hamming(ka["desc"], kb["desc"])
        rq, _ = oracle.ratio_filter(idx, dist, PM.FINISH_RATIO)
        assert len(rq) == M and len(ka["xy"]) >= 8, (name, len(rq), len(ka["xy"]))
    assert PM.FINISH_SEEDS["too_few"][1] < 6 == PM.FINISH_SEEDS["six"][1] and PM.FINISH_SEEDS["eight"][1] == 8
