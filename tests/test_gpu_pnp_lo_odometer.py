"""StereoOdometer(pnp_lo_rounds=3) on the GPU: 12 C1 pairs (frames 0 - 12), depth="sparse", pnp_refine=3.

    pairwise    update() equals the CPU chain (pnp_lo_ref.LoRefOdometer: the restatement on the oracle's ORB, matching and RANSAC) in
                accept flags, skip_cause and skipped_frames, c_T_w to 1e-9 -- the bar the sparse odometer is held to the plain CPU
                chain with; run() equals update() in c_T_w, accept flags and skip_cause with np.array_equal; every pair is one
                pnp_pair_lo (update) or one pnp_pair_begin_lo / pnp_pair_end_lo (run), never a plain entry
    map         track="map" unfused against map_fused=True: every decision and count equal, c_T_w to 1e-9 (the bar of
                tests/test_gpu_map_fused.py); the fused frames are ONE track_map_lo each; pnp_lo_counts is set
    rounds 0    the same odometer without the keyword makes none of the new calls (tests/test_pnp_lo_ref.py scripts the rest)
    keywords    depth="dense", cross_check, match_window and loop_check with rounds on 5 frames: the same entries, run() == update()"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_lo_ref as PL                    # noqa: E402

pytestmark = pytest.mark.gpu

N_FRAMES = 13
BASE = dict(preprocessed_frames=True, depth="sparse", pose_method="pnp", pnp_refine=3)
LO_CALLS = ("pnp_pair_lo", "pnp_pair_begin_lo", "pnp_pair_end_lo", "track_map_lo")
PLAIN_CALLS = ("pnp_pair", "pnp_pair_window", "pnp_pair_begin", "pnp_pair_begin_window", "pnp_pair_end", "map_track")


@pytest.fixture(scope="module")
def c1():
    from openvo_amd import StereoCamera, _native
    from openvo_amd.synth import Corridor
    ctx = _native.Context(0, 640, 480, 64, 500)
    c = Corridor("C1")
    cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), context=ctx)
    yield dict(ctx=ctx, cam=cam, frames=c.pairs(0, N_FRAMES))
    ctx.close()


class _Counting:
    """counts the context's PnP / map-step calls by name while it is active"""

    def __init__(self, ctx):
        self.ctx, self.calls = ctx, {n: 0 for n in LO_CALLS + PLAIN_CALLS}

    def __enter__(self):
        for n in self.calls:
            real = getattr(self.ctx, n)

            def f(*a, _real=real, _n=n, **k):
                self.calls[_n] += 1
                return _real(*a, **k)
            setattr(self.ctx, n, f)
        return self

    def __exit__(self, *exc):
        for n in self.calls:
            delattr(self.ctx, n)

    def used(self):
        return {n: v for n, v in self.calls.items() if v}


def _chain(odo, frames):
    return [(odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()) for L, R in frames]


def test_pairwise_update_run_and_the_cpu_chain(oracle, c1):
    from openvo_amd import StereoOdometer
    from openvo_amd.synth import Corridor
    ctx, cam, frames = c1["ctx"], c1["cam"], c1["frames"]
    ref = PL.LoRefOdometer(oracle, cam.Q, cam.valid_region_left, frames={}, refine=3, rounds=3)
    want = _chain(ref, frames)
    with _Counting(ctx) as cnt:
        odo = StereoOdometer(cam, pnp_lo_rounds=3, **BASE)
        got, lo = [], []
        for L, R in frames:
            got.append((odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()))
            lo.append(odo.pnp_lo_counts)
        used = cnt.used()
    assert sum(w[0] for w in want) >= N_FRAMES - 2, [w[:3] for w in want]
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w[:3], (k, g[:3], w[:3])
        worst = max(worst, float(np.abs(g[3] - w[3]).max()))
        assert np.allclose(g[3], w[3], rtol=0, atol=1e-9), (k, np.abs(g[3] - w[3]).max())
    assert set(used) <= {"pnp_pair_lo", "pnp_pair_begin_lo", "pnp_pair_end_lo"} and sum(used.values()) >= N_FRAMES - 1, used
    assert lo[0] is None and all(c is not None and c[0] == 3 and c[1] >= 10 for c, g in zip(lo[1:], got[1:]) if g[0]), lo
    with _Counting(ctx) as cnt:
        odo2 = StereoOdometer(cam, pnp_lo_rounds=3, **BASE)
        ran = [(ok, odo2.skip_cause, odo2.skipped_frames, odo2.c_T_w.copy()) for ok in odo2.run(iter(frames), depth=4)]
        used_run = cnt.used()
    assert len(ran) == len(got)
    for g, r in zip(got, ran):
        assert g[:3] == r[:3] and np.array_equal(g[3], r[3])
    assert set(used_run) <= {"pnp_pair_lo", "pnp_pair_begin_lo", "pnp_pair_end_lo"}, used_run
    # without the keyword: today's calls and none of the new ones; the poses differ (the rounds do something)
    with _Counting(ctx) as cnt:
        plain = _chain(StereoOdometer(cam, **BASE), frames)
        used_plain = cnt.used()
    assert not set(used_plain) & set(LO_CALLS), used_plain
    assert not np.array_equal(plain[-1][3], got[-1][3])
    gt = np.linalg.inv(Corridor.gt_pose(0)) @ Corridor.gt_pose(N_FRAMES - 1)
    err = [float(np.linalg.norm(np.linalg.inv(T)[:3, 3] - gt[:3, 3])) for T in (plain[-1][3], got[-1][3])]
    print("12 C1 pairs, seed 4321: end-point error refine 3 %.4f m, 3 x 3 %.4f m; largest |c_T_w - CPU chain| %.3g; calls %s (update), %s (run)" % (
        err[0], err[1], worst, used, used_run))
    assert ctx.sgbm_sweep_status() == 0


def test_map_unfused_against_fused(c1):
    from openvo_amd import StereoOdometer
    ctx, cam, frames = c1["ctx"], c1["cam"], c1["frames"]

    def chain(**kw):
        odo = StereoOdometer(cam, track="map", pnp_lo_rounds=3, **dict(BASE, **kw))
        out = []
        with _Counting(ctx) as cnt:
            for L, R in frames:
                ok = odo.update(L, R)
                out.append((ok, odo.skip_cause, odo.skipped_frames, odo.track_source, odo.c_T_w.copy(),
                            {n: tuple(int(x) for x in v) for n, v in odo.map_counts.items()}, odo.pnp_lo_counts))
        lm = odo.landmarks()
        odo.release_map()
        return out, cnt.used(), lm
    unfused, used_u, lm_u = chain()
    fused, used_f, lm_f = chain(map_fused=True)
    for k, (u, f) in enumerate(zip(unfused, fused)):
        assert u[:4] == f[:4] and u[5] == f[5] and u[6] == f[6], (k, u[:4], f[:4], u[5], f[5], u[6], f[6])
        assert np.abs(u[4] - f[4]).max() <= 1e-9, (k, np.abs(u[4] - f[4]).max())
    assert sum(f[3] == "map" for f in fused) >= N_FRAMES - 3, [f[3] for f in fused]
    assert used_f.get("track_map_lo") == N_FRAMES - 1 and not set(used_f) & set(PLAIN_CALLS), used_f       # one call per map step
    assert used_u.get("pnp_pair_lo", 0) >= N_FRAMES - 1 and not set(used_u) & set(PLAIN_CALLS + ("track_map_lo",)), used_u
    assert all(f[6] is not None and f[6][0] == 3 for f in fused[1:] if f[3] == "map")
    for n in ("desc", "octave", "obs", "last"):
        assert np.array_equal(lm_u[n], lm_f[n]), n
    assert np.abs(lm_u["xyz"] - lm_f["xyz"]).max() <= 1e-5
    print("map of %d landmarks; last (rounds, support) %s" % (len(lm_f["xyz"]), fused[-1][6]))


@pytest.mark.parametrize("name,kw", [("dense", dict()), ("dense-cross-window", dict(cross_check=True, match_window=(24, 16))),
                                     ("sparse-cross-window-loop", dict(depth="sparse", cross_check=True, match_window=(24, 16), loop_check=48))])
def test_rounds_compose_with_dense_depth_and_the_match_keywords(c1, name, kw):
    """5 C1 frames: with depth="dense" and with cross_check / match_window / loop_check the rounds run through the same entries
    (never a plain one), every accepted pair completes its 3 rounds, run() equals update(), and the poses differ from the same
    odometer without rounds while its decisions do not."""
    from openvo_amd import StereoOdometer
    ctx, cam, frames = c1["ctx"], c1["cam"], c1["frames"][:5]
    base = dict(preprocessed_frames=True, pose_method="pnp", pnp_refine=3, **kw)
    with _Counting(ctx) as cnt:
        odo = StereoOdometer(cam, pnp_lo_rounds=3, **base)
        got, lo = [], []
        for L, R in frames:
            got.append((odo.update(L, R), odo.skip_cause, odo.skipped_frames, odo.c_T_w.copy()))
            lo.append(odo.pnp_lo_counts)
        odo2 = StereoOdometer(cam, pnp_lo_rounds=3, **base)
        ran = [(ok, odo2.skip_cause, odo2.skipped_frames, odo2.c_T_w.copy()) for ok in odo2.run(iter(frames), depth=3)]
        used = cnt.used()
    assert sum(g[0] for g in got) >= 4, [g[:3] for g in got]
    assert set(used) <= {"pnp_pair_lo", "pnp_pair_begin_lo", "pnp_pair_end_lo"} and used.get("pnp_pair_lo", 0) >= 4, used
    assert all(c is not None and c[0] == 3 and c[1] >= 10 for c, g in zip(lo[1:], got[1:]) if g[0]), lo
    for g, r in zip(got, ran):
        assert g[:3] == r[:3] and np.array_equal(g[3], r[3])
    plain = _chain(StereoOdometer(cam, **base), frames)
    assert [p[:3] for p in plain] == [g[:3] for g in got] and not np.array_equal(plain[-1][3], got[-1][3])
    print("%s: calls %s, (rounds, support) per frame %s" % (name, used, lo[1:]))
    assert ctx.sgbm_sweep_status() == 0
