"""The dense direct alignment on a C2 stream (1280x720, 500 features, dense depth, host pairs), one GPU, ONE process: the step alone
(Context.direct_align on two slots of the stream, from the identity: wall time of the synchronous call -- pyramid launches, the one
k_direct_align launch, the synchronisation -- and the library's event bracket around the kernel, median of --step-calls calls after
10 warm-up calls, at the default 16384 points per level and at 65536); then frames per second of synchronous
StereoOdometer.update() loops and of StereoOdometer.run() with and without direct_refine, for both pose methods, the modes
alternating inside every round.  Prints one JSON line.  Needs a GPU: there is no fallback.  Reads nothing but the package (the
synthetic corridor).

    python tools/bench_direct.py [--pairs 240] [--rounds 3] [--step-calls 200]

--affine: the step alone and nothing else, plain (vo_direct_align) and affine (vo_direct_align_ab: a gain and an offset estimated beside
the pose) ALTERNATING inside every one of --rounds rounds of the same process, at both point counts; per round the medians of both and
the ratio affine / plain of that round.

--keypoints: the PATCH alignment of sparse stereo depth (Context.direct_align_kp, StereoOdometer(depth="sparse", patch_refine=True)).
The step alone on two sparse slots of the stream, from the identity, at the odometer's defaults (3 levels x 4 iterations, patch 5),
ALTERNATING with the dense step (3 x 8, 16384 points) on two dense slots inside every one of --rounds rounds: call time, kernel time,
keypoints and points per level.  Then frames per second of synchronous update() loops and of run() in sparse mode with and without
patch_refine, both pose methods, the modes alternating inside every round."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=240, help="pairs per timed pass")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per mode, after one warm-up pass")
ap.add_argument("--step-calls", type=int, default=200, help="timed calls of the step per point count")
ap.add_argument("--affine", action="store_true", help="the step alone, plain and affine alternating in every round")
ap.add_argument("--keypoints", action="store_true", help="the patch alignment of sparse stereo depth: the step beside the dense one, then the sparse loops")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
frames = c.pairs(0, 48)
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
ctx = cam._ctx
result = {"tool": "bench_direct", "device": ctx.device_name()}
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]
Q = cam.Q
K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]


def stats(v):
    return {"median": round(float(np.median(v)), 1), "p10": round(float(np.percentile(v, 10)), 1), "p90": round(float(np.percentile(v, 90)), 1)}


# ---------------------------------------------------------------------------------------------- the step alone
def timed_step(sa, sb, n, **kw):
    """median / p10 / p90 of --step-calls synchronous calls after 10 warm-up calls: the call's wall time and the kernel's event bracket"""
    wall, kern, r = [], [], None
    for step in range(-10, args.step_calls):
        ctx.enable_timing(step >= 0)
        t0 = time.perf_counter()
        r = ctx.direct_align(sa, sb, K4, max_points=n, dmin=StereoOdometer.MIN_VALID_DISPARITY, dmax=StereoOdometer.MAX_VALID_DISPARITY, **kw)
        dt = 1e6 * (time.perf_counter() - t0)
        if step < 0:
            continue
        t = ctx.timings(reset=True)
        wall.append(dt)
        kern.append(1e3 * t["pose"][0])
    ctx.enable_timing(False)
    out = dict(status=r["status"], iters_done=r["iters_done"], s=r["s"].tolist(), selected=r["selected"].tolist(),
               participants_last=r["n_last"].tolist(), call_us=stats(wall), kernel_us=stats(kern))
    if "gain" in r:
        out.update(gain=round(r["gain"], 5), offset=round(r["offset"], 4), unknowns=r["unknowns"])
    return out


def step_slots():
    x3a, _, _ = cam.compute_3d(*stream[0], preprocessed=True)
    x3b, _, _ = cam.compute_3d(*stream[1], preprocessed=True)
    return x3a.frame.slot, x3b.frame.slot


def step_alone():
    sa, sb = step_slots()
    return {str(n): timed_step(sa, sb, n) for n in (16384, 65536)}


def step_plain_and_affine():
    sa, sb = step_slots()
    out = {}
    for n in (16384, 65536):
        rounds = []
        for _ in range(args.rounds):                   # plain and affine alternate inside every round
            plain, affine = timed_step(sa, sb, n), timed_step(sa, sb, n, affine=True)
            rounds.append(dict(plain=plain, affine=affine,
                               kernel_affine_over_plain=round(affine["kernel_us"]["median"] / plain["kernel_us"]["median"], 3),
                               call_affine_over_plain=round(affine["call_us"]["median"] / plain["call_us"]["median"], 3)))
        out[str(n)] = rounds
    return out


if args.affine:
    result["workload"] = "C2 1280x720, two slots of the stream, from the identity, 3 levels x 8 iterations (synthetic corridor, one GPU)"
    result["rounds"] = args.rounds
    result["step_plain_and_affine"] = step_plain_and_affine()
    ctx.close()
    print(json.dumps(result))
    sys.exit(0)


def timed_step_kp(sa, sb, **kw):
    """timed_step for the patch alignment (Context.direct_align_kp)"""
    wall, kern, r = [], [], None
    for step in range(-10, args.step_calls):
        ctx.enable_timing(step >= 0)
        t0 = time.perf_counter()
        r = ctx.direct_align_kp(sa, sb, K4, **kw)
        dt = 1e6 * (time.perf_counter() - t0)
        if step < 0:
            continue
        t = ctx.timings(reset=True)
        wall.append(dt)
        kern.append(1e3 * t["pose"][0])
    ctx.enable_timing(False)
    return dict(status=r["status"], iters_done=r["iters_done"], patch=r["patch"], keypoints=r["keypoints"].tolist(), selected=r["selected"].tolist(),
                participants_last=r["n_last"].tolist(), call_us=stats(wall), kernel_us=stats(kern))


def step_keypoints_and_dense():
    da, db = step_slots()
    ka = cam.compute_sparse(*stream[0], 500, preprocessed=True)[2].frame.slot
    kb = cam.compute_sparse(*stream[1], 500, preprocessed=True)[2].frame.slot
    rounds = []
    for _ in range(args.rounds):                       # the patch step and the dense step alternate inside every round
        kp, dense = timed_step_kp(ka, kb), timed_step(da, db, 16384)
        rounds.append(dict(keypoints=kp, dense=dense, kernel_keypoints_over_dense=round(kp["kernel_us"]["median"] / dense["kernel_us"]["median"], 3),
                           call_keypoints_over_dense=round(kp["call_us"]["median"] / dense["call_us"]["median"], 3)))
    return rounds


# ---------------------------------------------------------------------------------------------- the loops
BASE = dict(nfeatures=500, preprocessed_frames=True)
if args.keypoints:
    result["step_keypoints_and_dense"] = step_keypoints_and_dense()
    MODES = {"umeyama": dict(depth="sparse"), "umeyama_patch": dict(depth="sparse", patch_refine=True),
             "pnp": dict(depth="sparse", pose_method="pnp"), "pnp_patch": dict(depth="sparse", pose_method="pnp", patch_refine=True)}
    REFINED, WORKLOAD = "_patch", "sparse depth, %d host pairs per pass (synthetic corridor, one GPU); patch_refine at its defaults (3 x 4, patch 5)"
else:
    result["step"] = step_alone()
    MODES = {"umeyama": dict(rigidity_threshold=0.1, outlier_threshold=0.02), "umeyama_direct": dict(rigidity_threshold=0.1, outlier_threshold=0.02, direct_refine=True),
             "pnp": dict(pose_method="pnp"), "pnp_direct": dict(pose_method="pnp", direct_refine=True)}
    REFINED, WORKLOAD = "_direct", ("dense depth, %d host pairs per pass (synthetic corridor, one GPU); umeyama with the clique "
                                    "and outlier filters (0.1, 0.02)")

def one_pass(kw, run):
    odo = StereoOdometer(cam, **BASE, **kw)
    ctx.synchronize()
    accepted = taken = 0
    t0 = time.perf_counter()
    for ok in (odo.run(iter(stream)) if run else (odo.update(L, R) for L, R in stream)):
        accepted += bool(ok)
        taken += bool(ok and ((odo.direct_refine and odo.direct_accepted) or (odo.patch_refine and odo.patch_accepted)))
    ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    return len(stream) / dt, accepted, taken


def report(rates):
    return {k: {"per_round": [round(x[0], 1) for x in v], "median": round(float(np.median([x[0] for x in v])), 1),
                "accepted": [x[1] for x in v], "refined_poses_taken": [x[2] for x in v]} for k, v in rates.items()}


result["workload"] = "C2 1280x720, 500 features, " + WORKLOAD % len(stream)
result["rounds"] = args.rounds
for name, run in (("update_frames_per_s", False), ("run_frames_per_s", True)):
    for kw in MODES.values():
        one_pass(kw, run)                              # warm-up: allocations, clocks
    rates = {k: [] for k in MODES}
    for r in range(args.rounds):                       # the modes alternate inside every round
        for k, kw in MODES.items():
            rates[k].append(one_pass(kw, run))
    result[name] = report(rates)
    for m in ("umeyama", "pnp"):
        result[name][m + REFINED + "_over_plain_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(rates[m + REFINED], rates[m])]
ctx.close()
print(json.dumps(result))
