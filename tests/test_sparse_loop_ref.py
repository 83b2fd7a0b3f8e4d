"""The association tests (mutual, ratio) of the sparse stereo chain and the temporal loop check on the CPU: known answers for the
numpy restatement tests/sparse_loop_ref.py, the restatement on the oracle's ORB of C1 frames 0-7 against the oracle's SGBM, the CPU
odometer chain with the loop gate, and the host logic of the new public arguments."""
import os
import re

import numpy as np
import pytest

import sparse_loop_ref as X
import sparse_stereo_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (4, 100, 2.0, 75)


def _flip(d, bits):
    """descriptor d with the given bit positions flipped"""
    u = np.unpackbits(np.asarray(d, np.uint8).reshape(32))
    u[list(bits)] ^= 1
    return np.packbits(u)


def _base(seed=0):
    return np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)


def _row(xs, y=30.0):
    return np.stack([np.asarray(xs, np.float32), np.full(len(xs), y, np.float32)], 1)


# ---- known answers --------------------------------------------------------------------------------------------------------------
def test_two_left_keypoints_with_the_same_best():
    """Left 0 and 1 both have right 0 as their only candidate: the smaller (distance, i) keeps it."""
    b = _base()
    xy_l, xy_r = _row([50, 52]), _row([40])
    o = np.zeros(2, np.int32)
    # left 1 is nearer (3 bits against 5)
    m, a = X.associate_ex(xy_l, o, [_flip(b, range(5)), _flip(b, range(3))], xy_r, [0], [b], *PARAMS, flags=X.MUTUAL)
    assert list(m) == [-1, 0] and int(a[0]) == (3 << 16 | 1)
    # equal distances: the lower i
    m, a = X.associate_ex(xy_l, o, [_flip(b, range(4)), _flip(b, range(4, 8))], xy_r, [0], [b], *PARAMS, flags=X.MUTUAL)
    assert list(m) == [0, -1] and int(a[0]) == (4 << 16 | 0)
    # without the test both keep it
    m, _ = X.associate_ex(xy_l, o, [_flip(b, range(4)), _flip(b, range(4, 8))], xy_r, [0], [b], *PARAMS, flags=0)
    assert list(m) == [0, 0]


def test_a_better_claimant_whose_winner_is_elsewhere_still_defeats_the_claim():
    """Left 0: right 0 at distance 10 (its only candidate).  Left 1: right 0 at distance 4 and right 1 at distance 2 -- its
    winner is right 1, yet a(0) names left 1, so left 0 loses right 0 and nobody holds it."""
    b0, b1 = _base(1), _base(2)
    assert S.hamming(b0, b1)[0] > 100
    # left 1's descriptor: 2 bits from b1; right 0 is built 4 bits from left 1
    l1 = _flip(b1, range(2))
    r0 = _flip(l1, range(10, 14))
    l0 = _flip(r0, range(20, 30))
    xy_l = _row([50, 60])
    xy_r = _row([45, 55])             # left 0: only right 0 in [4, 100] (50 - 55 < 0); left 1: both
    m, a = X.associate_ex(xy_l, [0, 0], [l0, l1], xy_r, [0, 0], [r0, b1], *PARAMS, flags=X.MUTUAL)
    assert int(a[0]) == (4 << 16 | 1) and int(a[1]) == (2 << 16 | 1)
    assert list(m) == [-1, 1]
    assert list(X.associate_ex(xy_l, [0, 0], [l0, l1], xy_r, [0, 0], [r0, b1], *PARAMS, flags=0)[0]) == [0, 1]


def test_ratio_known_answers():
    b = _base(3)
    xy_l, xy_r = _row([60]), _row([50, 48])
    # d1 == d2 fails at ratio 1 (the comparison is strict)
    m, _ = X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], [_flip(b, range(6)), _flip(b, range(6, 12))], *PARAMS, flags=X.RATIO, ratio=1.0)
    assert list(m) == [-1]
    # 6 against 7 passes at ratio 1, fails at 0.8 (6 < 5.6 is false), and 4 against 6 passes at 0.8 (4 < 4.8)
    two = [_flip(b, range(6)), _flip(b, range(6, 13))]
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], two, *PARAMS, flags=X.RATIO, ratio=1.0)[0]) == [0]
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], two, *PARAMS, flags=X.RATIO, ratio=0.8)[0]) == [-1]
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], [_flip(b, range(4)), _flip(b, range(6, 12))], *PARAMS, flags=X.RATIO, ratio=0.8)[0]) == [0]
    # a single candidate passes
    assert list(X.associate_ex(xy_l, [0], [b], xy_r[:1], [0], two[:1], *PARAMS, flags=X.RATIO, ratio=0.5)[0]) == [0]
    # a second candidate above max_hamming still counts as the runner-up: 70 against 80 at ratio 0.8 (70 < 64 is false), max_hamming 75
    far = [_flip(b, range(70)), _flip(b, range(100, 180))]
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], far, *PARAMS, flags=X.RATIO, ratio=0.8)[0]) == [-1]
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], far, *PARAMS, flags=0)[0]) == [0]
    # ... and a winner above max_hamming fails whatever the ratio says
    assert list(X.associate_ex(xy_l, [0], [b], xy_r, [0, 0], [_flip(b, range(80)), _flip(b, range(56, 256))], *PARAMS, flags=X.RATIO, ratio=1.0)[0]) == [-1]


def test_flags_zero_is_the_plain_association():
    rng = np.random.default_rng(11)
    nl, nr = 150, 120
    xy_l = np.stack([rng.uniform(0, 96, nl), rng.uniform(0, 64, nl)], 1).astype(np.float32)
    xy_r = np.stack([rng.uniform(0, 96, nr), rng.uniform(0, 64, nr)], 1).astype(np.float32)
    o_l, o_r = rng.integers(0, 8, nl), np.sort(rng.integers(0, 8, nr))
    d_l = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    d_r = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    for mh in (75, 120, 256):
        want = S.associate(xy_l, o_l, d_l, xy_r, o_r, d_r, 4, 100, 2.0, mh)
        got, a = X.associate_ex(xy_l, o_l, d_l, xy_r, o_r, d_r, 4, 100, 2.0, mh, flags=0)
        assert np.array_equal(got, want) and got.dtype == want.dtype
    assert (want >= 0).sum() > 20
    # every test only ever removes associations
    for fl in (1, 2, 3):
        got, _ = X.associate_ex(xy_l, o_l, d_l, xy_r, o_r, d_r, 4, 100, 2.0, 256, flags=fl, ratio=0.9)
        assert ((got == want) | (got == -1)).all() and (got >= 0).sum() < (want >= 0).sum()
    with pytest.raises(ValueError):
        X.associate_ex(np.zeros((65537, 2), np.float32), np.zeros(65537), np.zeros((65537, 32), np.uint8), xy_r, o_r, d_r, 4, 100, 2.0, 75, flags=1)


# ---- C1 frames 0-7 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1(oracle):
    from openvo_amd import calib
    from openvo_amd.synth import Corridor
    c = Corridor("C1")
    Q, roi = calib.stereo_rectify(c.K(), c.dist(), c.K(), c.dist(), (c.w, c.h), c.rect_params()["R"], c.rect_params()["T"])[4:6]
    frames = c.pairs(0, 8)
    x0, y0, x1, y1 = S.crop_bounds(roi, c.w, c.h)
    orb = [tuple(oracle.orb_detect_and_compute(np.ascontiguousarray(im[y0:y1, x0:x1]), None, 500) for im in pair) for pair in frames]
    dense = [oracle.sgbm_compute(L, R, c.sgbm_params()).astype(np.float32) / 16 for L, R in frames]
    return dict(c=c, Q=Q, roi=roi, frames=frames, orb=orb, dense=dense, origin=(x0, y0), crop=(x0, y0, x1, y1))


def _frame(c1, k, flags, ratio):
    x0, y0, x1, y1 = c1["crop"]
    L, R = c1["frames"][k]
    f = X.sparse_stereo_ex(np.ascontiguousarray(L[y0:y1, x0:x1]), np.ascontiguousarray(R[y0:y1, x0:x1]), c1["orb"][k][0], c1["orb"][k][1],
                           c1["Q"], x0, y0, *PARAMS, flags=flags, ratio=ratio)
    f["origin"] = (x0, y0)
    return f


def test_c1_association_tests_against_the_oracle_sgbm(c1):
    """Mutual + ratio 0.8 over C1 frames 0-7: at least 200 keypoints kept in every frame and at most 1 in total more than 1 px off
    the oracle's SGBM disparity (today's association: 3).  The full table is printed."""
    rows = {}
    for name, fl, r in (("today", 0, None), ("mutual", 1, None), ("ratio 0.8", 2, 0.8), ("mutual + ratio 0.8", 3, 0.8)):
        kept, gross, total = [], 0, 0
        for k in range(8):
            f = _frame(c1, k, fl, r)
            px = np.rint(f["xy"]).astype(int) + list(c1["origin"])
            dense = c1["dense"][k][px[:, 1], px[:, 0]]
            valid = (dense >= 4) & (dense <= 100)
            gross += int((np.abs(f["disp"][valid] - dense[valid]) > 1).sum())
            total += int(valid.sum())
            kept.append(int(f["counts3"][2]))
            assert np.array_equal(f["rdesc"], c1["orb"][k][1]["desc"][f["match"][f["keep"]]])
        rows[name] = (kept, gross, total)
        print("%-20s kept per frame %.0f (min %d), more than 1 px off the oracle's SGBM: %d of %d" % (name, np.mean(kept), min(kept), gross, total))
    kept, gross, _ = rows["mutual + ratio 0.8"]
    assert min(kept) >= 200, kept
    assert gross <= 1, gross
    assert rows["today"][1] >= gross


def _chain(oracle, c1, loop_check, mutual=False, ratio=None, **kw):
    from openvo_amd.synth import Corridor
    fl = (1 if mutual else 0) | (2 if ratio is not None else 0)
    cache = {id(L): _frame(c1, k, fl, ratio) for k, (L, _) in enumerate(c1["frames"])}
    odo = X.SparseLoopOdometer(oracle, c1["Q"], c1["roi"], frames=cache, mutual=mutual, ratio=ratio, loop_check=loop_check, **kw)
    oks = [odo.update(L, R) for L, R in c1["frames"]]
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(len(c1["frames"]) - 1)
    return oks, float(np.linalg.norm(odo.current_pose()[:3, 3] - gt[:3, 3])), odo


def test_c1_loop_check_rescues_the_default_odometer(oracle, c1):
    """Default odometer (no filters), today's association, over C1 frames 0-7: with loop_check = 48 every pair is accepted and the
    end-point error is at most one third of the same chain's without it.  The full table is printed; a threshold of 256 changes
    nothing."""
    table = {}
    for name, kw in (("default (no filters)", {}), ("clique + outlier (0.1 / 0.02)", dict(rigidity_threshold=0.1, outlier_threshold=0.02)),
                     ("PnP (256, 1.5, 4321)", dict(pose_method="pnp"))):
        table[name] = [_chain(oracle, c1, lc, **kw) for lc in (None, 48, 64)]
        print("%-30s no loop check %.3f m, loop <= 48 %.3f m, loop <= 64 %.3f m" % (name, *[e for _, e, _ in table[name]]))
    oks, e_both, _ = _chain(oracle, c1, None, mutual=True, ratio=0.8, rigidity_threshold=0.1, outlier_threshold=0.02)
    print("clique + outlier with mutual + ratio 0.8: %.3f m" % e_both)
    (_, e_plain, o_plain), (oks48, e48, _), _ = table["default (no filters)"]
    assert all(oks48), oks48
    assert e48 <= e_plain / 3, (e48, e_plain)
    _, e256, o256 = _chain(oracle, c1, 256)
    assert e256 == e_plain and o256.log == o_plain.log


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_association_state_validation():
    from openvo_amd._native import sparse_assoc_state
    assert sparse_assoc_state() == (0, 0.0)
    assert sparse_assoc_state(True, None) == (1, 0.0)
    assert sparse_assoc_state(False, 1) == (2, 1.0)
    assert sparse_assoc_state(True, 0.8) == (3, float(np.float32(0.8)))
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), "0.8", True, (0.8,)):
        with pytest.raises(ValueError):
            sparse_assoc_state(False, bad)
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError):
            sparse_assoc_state(bad, None)


def test_sparse_request_validates_the_association_keywords():
    from openvo_amd.stereo_camera import sparse_request
    assert sparse_request(500) == sparse_request(500, mutual=False, assoc_ratio=None)
    assert sparse_request(500, mutual=True, assoc_ratio=0.8) != sparse_request(500)
    assert sparse_request(500, mutual=True) != sparse_request(500, assoc_ratio=0.8)
    for bad in (0, -1, 1.01, float("nan"), "0.8", True):
        with pytest.raises(ValueError):
            sparse_request(500, assoc_ratio=bad)
    for bad in (None, 1, "no"):
        with pytest.raises(ValueError):
            sparse_request(500, mutual=bad)


def test_odometer_validates_the_association_arguments():
    from openvo_amd import StereoOdometer

    class _Cam:
        _ctx = None
    odo = StereoOdometer(_Cam(), depth="sparse", sparse_mutual=True, sparse_ratio=0.8)
    assert (odo.sparse_mutual, odo.sparse_ratio) == (True, 0.8)
    assert StereoOdometer(_Cam()).sparse_mutual is False and StereoOdometer(_Cam()).sparse_ratio is None
    for bad in (0, 1.5, -1, float("nan"), "0.8", True):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="sparse", sparse_ratio=bad)
    for bad in (None, 1, "yes"):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="sparse", sparse_mutual=bad)
    for kw in (dict(sparse_mutual=True), dict(sparse_ratio=0.8)):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="dense", **kw)


def test_loop_check_validation():
    """loop_check of the odometer, _native.loop_threshold and Context.set_match_loop: None or an int in 0 .. 256, nothing else;
    depth="dense" refuses it"""
    from openvo_amd import StereoOdometer, _native

    class _Cam:
        _ctx = None
    assert StereoOdometer(_Cam()).loop_check is None and StereoOdometer(_Cam(), depth="sparse").loop_check is None
    for good in (0, 48, 256, np.int32(64)):
        odo = StereoOdometer(_Cam(), depth="sparse", loop_check=good)
        assert odo.loop_check == int(good) and type(odo.loop_check) is int
        assert _native.loop_threshold(good) == int(good)
    assert _native.loop_threshold(None) is None
    for bad in (-1, 257, 48.0, True, False, "48", (48,), float("nan")):
        with pytest.raises(ValueError):
            StereoOdometer(_Cam(), depth="sparse", loop_check=bad)
        with pytest.raises(ValueError):
            _native.loop_threshold(bad)
    for d in ({}, dict(depth="dense")):
        with pytest.raises(ValueError, match="sparse"):
            StereoOdometer(_Cam(), loop_check=48, **d)
    assert StereoOdometer(_Cam(), depth="dense", loop_check=None).loop_check is None

    class _Lib:
        calls = []

        def vo_set_match_loop(self, h, n):
            self.calls.append(("set", n))
            return 0

        def vo_clear_match_loop(self, h):
            self.calls.append(("clear",))
            return 0

    class _Self:                                # Context's methods on a stand-in: the wrapper's own logic, no device
        _lib, _h, _loop = _Lib(), None, None
        _ck = staticmethod(lambda rc: None)
        set_match_loop = _native.Context.set_match_loop
    me = _Self()
    for bad in (None, -1, 257, 48.0, True, "48"):
        with pytest.raises(ValueError):
            _native.Context.set_match_loop(me, bad)
    assert me._lib.calls == [] and me._loop is None
    _native.Context.set_match_loop(me, 48)
    _native.Context.set_match_loop(me, 48)                                    # the value in force: no native call
    assert me._lib.calls == [("set", 48)] and me._loop == 48
    assert _native.Context._mflags(me, True, None, 48) == 1 | 4 and _native.Context._mflags(me, False, None) == 0
    assert _native.Context._mflags(me, False, None, 0) == 4 and me._lib.calls == [("set", 48), ("set", 0)]
    _native.Context.clear_match_loop(me)
    assert me._loop is None and me._lib.calls[-1] == ("clear",)


def test_pose_step_key_carries_the_loop_check():
    """the threshold is a named entry of the key of a step begun ahead, behind the window where there is one, and reaches the
    native step as the keyword `loop` (the PnP step through its _window form)"""
    from openvo_amd import StereoOdometer
    from openvo_amd.stereo_odometer import LoopCheck

    class _Cam:
        _ctx = None
        Q = np.array([[1, 0, 0, -320.0], [0, 1, 0, -240.0], [0, 0, 0, 500.0], [0, 0, 2.0, 0]])
    plain = StereoOdometer(_Cam(), depth="sparse")._pose_params()
    odo = StereoOdometer(_Cam(), depth="sparse", loop_check=48)
    assert odo._pose_params() == plain + (LoopCheck(48),) and odo._split_loop(odo._pose_params()) == (plain, {"loop": 48})
    assert odo._split_loop(plain) == (plain, {}) and odo._loop_kw() == {"loop": 48}
    win = StereoOdometer(_Cam(), depth="sparse", loop_check=0, match_window=(24, 16))
    key = win._pose_params()
    assert key[-2] == (24.0, 16.0) and key[-1] == LoopCheck(0) and win._split_loop(key) == (key[:-1], {"loop": 0})
    assert win._split_loop(key[:-1]) == (key[:-1], {})                        # a window alone is never taken for a threshold
    pnp = StereoOdometer(_Cam(), depth="sparse", pose_method="pnp", loop_check=48)
    kw = pnp._pnp_kwargs(pnp._pose_params())
    assert kw["loop"] == 48 and kw["window"] is None
    kw = StereoOdometer(_Cam(), depth="sparse", pose_method="pnp", loop_check=48, match_window=8)._pnp_kwargs(
        StereoOdometer(_Cam(), depth="sparse", pose_method="pnp", loop_check=48, match_window=8)._pose_params())
    assert kw["loop"] == 48 and kw["window"] == (8.0, 8.0)
    kw = StereoOdometer(_Cam(), depth="sparse", pose_method="pnp")._pnp_kwargs(StereoOdometer(_Cam(), depth="sparse", pose_method="pnp")._pose_params())
    assert "loop" not in kw and "window" not in kw


def test_submit_request_carries_the_association_tests():
    """StereoCamera.submit_request on a scripted context: the tests go into the context ahead of the look-ahead entry (once), the
    SubmittedPair remembers the seven-entry request, a request without tests makes no association call, a bad one nothing at all"""
    from openvo_amd import StereoCamera, _native
    from openvo_amd.stereo_camera import _RESERVED, sparse_request

    class _Ctx:
        def __init__(self):
            self.calls, self._sparse_assoc = [], (0, 0.0)

        def set_sparse_assoc(self, mutual=False, ratio=None):
            self.calls.append(("set_sparse_assoc", mutual, ratio))
            self._sparse_assoc = _native.sparse_assoc_state(mutual, ratio)

        def prefetch_pair_sparse(self, slot, left, right, preprocessed, *req):
            self.calls.append(("prefetch_pair_sparse", slot, preprocessed) + req)
            return 64, 48

    cam = StereoCamera.__new__(StereoCamera)
    cam._ctx = _Ctx()
    cam._slot_owner, cam._slot_gen, cam._next_slot = [None] * _native.VO_NUM_SLOTS, [0] * _native.VO_NUM_SLOTS, 0
    cam._lookahead, cam._n_staged, cam.lookahead, cam.lookahead_stop = [], 0, 0, None
    img = np.zeros((48, 64), np.uint8)
    req = sparse_request(300, mutual=True, assoc_ratio=0.8)
    assert len(req) == 7 and req[5:] == (True, float(np.float32(0.8)))
    sp = cam.submit_request(img, img, req, preprocessed=True)
    assert sp.sparse == req and sp.slot is not None and cam._slot_owner[sp.slot] is _RESERVED
    assert [c[0] for c in cam._ctx.calls] == ["set_sparse_assoc", "prefetch_pair_sparse"]
    assert cam._ctx.calls[0][1:] == (True, req[6]) and cam._ctx.calls[1][1:] == (sp.slot, True) + req[:5]
    sp2 = cam.submit_request(img, img, req)
    assert [c[0] for c in cam._ctx.calls[2:]] == ["prefetch_pair_sparse"] and sp2.sparse == req        # the state in force: no call
    sp3 = cam.submit_request(img, img, sparse_request(300))
    assert sp3.sparse == (300, 4.0, 100.0, 2.0, 75) and cam._ctx.calls[3] == ("set_sparse_assoc", False, None)
    assert cam.submit_sparse(img, img, 300).sparse == sp3.sparse and len(cam._ctx.calls) == 6
    n = len(cam._ctx.calls)
    for bad in ((300, 4, 100, 2.0, 75, True, 1.5), (300, 4, 100, 2.0, 75, 1, None), (300, 4, 100, 2.0, 257), (300, 4, 100, 2.0, 75, True)[:0]):
        with pytest.raises((ValueError, TypeError)):
            cam.submit_request(img, img, bad)
    assert len(cam._ctx.calls) == n


def test_symbols_and_header_lines():
    from openvo_amd import _native
    header = open(os.path.join(ROOT, "include", "vo355.h")).read()
    names = ("vo_set_sparse_assoc", "vo_download_keypoint_rdesc", "vo_sparse_pair_host_ex", "vo_set_match_loop", "vo_clear_match_loop")
    for name in names:
        assert name in _native.SYMBOLS
        assert re.search(r"^int %s\(vo_ctx\* ctx[,)]" % name, header, re.M), name
    assert re.search(r"^#define VO_SPARSE_MUTUAL 1$", header, re.M) and re.search(r"^#define VO_SPARSE_RATIO 2$", header, re.M)
    assert re.search(r"^#define VO_MATCH_LOOP 4$", header, re.M) and _native.VO_MATCH_LOOP == 4
    for method in ("set_sparse_assoc", "download_keypoint_rdesc", "set_match_loop", "clear_match_loop"):
        assert callable(getattr(_native.Context, method))
    if os.path.exists(_native.LIB_PATH):
        lib = _native.lib()
        for name in names:
            assert hasattr(lib, name), name
