"""Host side of the sparse look-ahead: the binding, the argument validation of StereoCamera.submit_sparse and the kind checks on a
SubmittedPair (sparse pairs go to compute_sparse, dense ones to compute_3d), on a scripted context: no GPU."""
import inspect

import numpy as np
import pytest

from openvo_amd import StereoCamera, StereoOdometer, _native
from openvo_amd.stereo_camera import _RESERVED, SubmittedPair, sparse_request

ENTRIES = ("vo_prefetch_pair_sparse", "vo_prefetch_host_staged_sparse", "vo_prefetch_staged_pair_sparse", "vo_sparse_pair_host")
REQ = (300, 4.0, 100.0, 2.0, 75)


def test_binding_has_the_sparse_lookahead_entries():
    for name in ENTRIES:
        assert name in _native.SYMBOLS
    for name in ("prefetch_pair_sparse", "prefetch_host_staged_sparse", "prefetch_staged_pair_sparse", "sparse_pair_host"):
        assert callable(getattr(_native.Context, name, None)), name
    sig = inspect.signature(StereoCamera.submit_sparse)
    assert list(sig.parameters)[1:] == ["img_left", "img_right", "nfeatures", "preprocessed", "min_disp", "max_disp", "row_tol", "max_hamming"]
    assert [sig.parameters[k].default for k in ("preprocessed", "min_disp", "max_disp", "row_tol", "max_hamming")] == [False, 4, 100, 2.0, 75]
    assert inspect.signature(StereoCamera.submit_staged).parameters["sparse"].default is None


def _bound(fn, *a, **kw):
    """the arguments as the REAL binding (_native.Context.<fn>) would receive them, defaults applied"""
    b = inspect.signature(getattr(_native.Context, fn)).bind(None, *a, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k != "self"}


class _Ctx:
    """stands in for _native.Context: remembers how it was asked, every call bound against the real method's signature"""

    def __init__(self):
        self.calls = []

    def _note(self, fn, *a, **kw):
        self.calls.append((fn, _bound(fn, *a, **kw)))

    def prefetch_pair_sparse(self, *a, **kw):
        self._note("prefetch_pair_sparse", *a, **kw)
        return 64, 48

    def prefetch_host_staged_sparse(self, *a, **kw):
        self._note("prefetch_host_staged_sparse", *a, **kw)
        return 64, 48

    def prefetch_host_staged(self, *a, **kw):
        self._note("prefetch_host_staged", *a, **kw)
        return 64, 48

    def prefetch_pair(self, *a, **kw):
        self._note("prefetch_pair", *a, **kw)
        return 64, 48

    def upload_pair(self, *a, **kw):
        self._note("upload_pair", *a, **kw)
        return 64, 48

    def host_stage_fetch(self, *a, **kw):
        self._note("host_stage_fetch", *a, **kw)
        return np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.uint8)

    def sparse_stereo(self, *a, **kw):
        self._note("sparse_stereo", *a, **kw)
        return np.array([9, 7, 5], np.int32)

    def lookahead_drop(self, slot):
        self.calls.append(("lookahead_drop", dict(slot=slot)))

    def sgbm_compute(self, *a, **kw):
        raise AssertionError("a sparse pair never reaches the SGBM")


def _camera():
    cam = StereoCamera.__new__(StereoCamera)
    cam._ctx = _Ctx()
    cam._slot_owner = [None] * _native.VO_NUM_SLOTS
    cam._slot_gen = [0] * _native.VO_NUM_SLOTS
    cam._next_slot = 0
    cam._lookahead, cam._n_staged, cam.lookahead, cam.lookahead_stop = [], 0, 0, None
    cam.valid_region_left = (2, 2, 60, 44)
    return cam


IMG = np.zeros((48, 64), np.uint8)


@pytest.mark.parametrize("kw", [dict(nfeatures=-1), dict(nfeatures=2.0), dict(nfeatures=True), dict(nfeatures="300"), dict(min_disp=-1), dict(min_disp=100),
                                dict(max_disp=float("inf")), dict(max_disp=float("nan")), dict(min_disp=None), dict(row_tol=-0.5),
                                dict(row_tol=float("nan")), dict(row_tol="2"), dict(max_hamming=257), dict(max_hamming=-1),
                                dict(max_hamming=75.0), dict(max_hamming=True)])
def test_submit_sparse_refuses_a_bad_request_before_anything_is_submitted(kw):
    cam = _camera()
    args = dict(nfeatures=300, min_disp=4, max_disp=100, row_tol=2.0, max_hamming=75)
    args.update(kw)
    with pytest.raises(ValueError):
        cam.submit_sparse(IMG, IMG, args.pop("nfeatures"), **args)
    with pytest.raises(ValueError):
        cam.submit_staged(0, 64, 48, 1, True, sparse=(kw.get("nfeatures", 300), args["min_disp"], args["max_disp"], args["row_tol"], args["max_hamming"]))
    assert cam._ctx.calls == [] and not any(o is _RESERVED for o in cam._slot_owner)


def test_sparse_request_is_what_the_library_compares():
    assert sparse_request(300) == REQ
    assert sparse_request(np.int64(300), np.float32(4), 100, np.float64(2), np.int32(75)) == REQ
    assert sparse_request(300, 4, 100, 0.3)[3] == float(np.float32(0.3))
    odo = StereoOdometer(None, nfeatures=300, depth="sparse", sparse_row_tol=0.3, sparse_max_hamming=60)
    odo.orb = type("O", (), {"nfeatures": 300})()
    assert odo._sparse_req() == (300, 4.0, 100.0, float(np.float32(0.3)), 60)


def test_submitted_pair_kinds():
    cam = _camera()
    sp = cam.submit_sparse(IMG, IMG, 300, preprocessed=True)
    fn, a = cam._ctx.calls[-1]
    assert fn == "prefetch_pair_sparse" and (a["slot"], a["preprocessed"]) == (sp.slot, True)
    assert (a["nfeatures"], a["min_disp"], a["max_disp"], a["row_tol"], a["max_hamming"]) == REQ
    assert sp.sparse == REQ and sp.shape == (64, 48) and cam._slot_owner[sp.slot] is _RESERVED
    dense = cam.submit(IMG, IMG, preprocessed=True)
    assert dense.sparse is None and cam._ctx.calls[-1][0] == "prefetch_pair"
    n = len(cam._ctx.calls)
    with pytest.raises(ValueError):
        cam.compute_3d(sp, None)
    with pytest.raises(ValueError):
        cam.compute_sparse(dense, None, 300)
    assert len(cam._ctx.calls) == n and cam._slot_owner[sp.slot] is _RESERVED and cam._slot_owner[dense.slot] is _RESERVED
    slot = sp.slot
    kps, desc, xyz, disp, left = cam.compute_sparse(sp, None, 300, preprocessed=True)
    fn, a = cam._ctx.calls[-1]
    assert fn == "sparse_stereo" and len(cam._ctx.calls) == n + 1                  # collected: nothing uploaded
    assert (a["slot"], a["nfeatures"], a["min_disp"], a["max_disp"], a["row_tol"], a["max_hamming"]) == (slot,) + (300, 4, 100, 2.0, 75)
    assert len(kps) == 5 and sp.slot is None and cam._slot_owner[slot]() is kps.frame
    with pytest.raises(ValueError):
        cam.compute_sparse(sp, None, 300)                                            # consumed
    # release works for both kinds, and twice
    sp2 = cam.submit_sparse(IMG, IMG, 300)
    for p in (sp2, dense, sp2):
        cam.release_submitted(p)
    assert [c for c in cam._ctx.calls if c[0] == "lookahead_drop"] == [("lookahead_drop", dict(slot=s)) for s in (2, 1)]
    assert not any(o is _RESERVED for o in cam._slot_owner)


def test_submit_staged_with_a_sparse_request():
    cam = _camera()
    sp = cam.submit_staged(3, 64, 48, 1, True, sparse=(300, 4, 100, 2.0, 75))
    fn, a = cam._ctx.calls[-1]
    assert fn == "prefetch_host_staged_sparse" and (a["buf"], a["w"], a["h"], a["ch"], a["preprocessed"]) == (3, 64, 48, 1, True)
    assert (a["nfeatures"], a["min_disp"], a["max_disp"], a["row_tol"], a["max_hamming"]) == REQ and sp.sparse == REQ
    d = cam.submit_staged(4, 64, 48, 1, True)
    assert cam._ctx.calls[-1][0] == "prefetch_host_staged" and d.sparse is None


def test_no_free_slot_keeps_a_sparse_pair_on_the_host():
    cam = _camera()
    for s in range(_native.VO_NUM_SLOTS - 3):
        cam._slot_owner[s] = _RESERVED
    L = np.full((48, 64), 7, np.uint8)
    sp = cam.submit_sparse(L, IMG, 300, preprocessed=True)
    assert sp.slot is None and sp.sparse == REQ and cam._ctx.calls == [] and sp.images[0] is not L and np.array_equal(sp.images[0], L)
    sp2 = cam.submit_staged(0, 64, 48, 1, True, sparse=REQ)
    assert sp2.slot is None and sp2.sparse == REQ and [c[0] for c in cam._ctx.calls] == ["host_stage_fetch"]
    with pytest.raises(ValueError):
        cam.compute_3d(sp, None)
    kps = cam.compute_sparse(sp, None, 300)[0]
    assert [c[0] for c in cam._ctx.calls[-2:]] == ["upload_pair", "sparse_stereo"] and cam._ctx.calls[-2][1]["preprocessed"] is True
    assert len(kps) == 5
    with pytest.raises(ValueError):
        cam.compute_sparse(sp, None, 300)


def test_a_failed_collection_gives_the_slot_back():
    cam = _camera()
    sp = cam.submit_sparse(IMG, IMG, 300)
    slot = sp.slot

    def boom(*a, **kw):
        raise _native.VoError(-4, "capacity")
    cam._ctx.sparse_stereo = boom
    with pytest.raises(_native.VoError):
        cam.compute_sparse(sp, None, 300)
    assert cam._slot_owner[slot] is None and cam._ctx.calls[-1] == ("lookahead_drop", dict(slot=slot))
    assert isinstance(sp, SubmittedPair) and sp.slot is None
