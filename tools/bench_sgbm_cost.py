"""The two SGBM matching costs side by side -- BT (Birchfield-Tomasi + SAD, OpenCV's: k_sgbm_planes + k_sgbm_cost_sweep) and census 9 x 7
(k_census + k_census_cost, csrc/sgbm_census.inc) -- on a C2 stream (1280x720, D = 128, mode 0, synthetic corridor, host pairs), the
costs alternating inside every round of ONE process:

    front_ms      the library's event bracket around the front of a synchronous pair (vo_get_timings: sgbm_cost = both kernels of
                  the cost in force), per round the median of --stage-calls calls; beside it sgbm_agg, sgbm_wta and sgbm_post, which
                  the cost does not touch
    compute_3d    pairs per second of a synchronous StereoCamera.compute_3d loop (one pair in flight: latency)
    run           frames per second of StereoOdometer.run() of the default odometer (500 features; pairs submitted ahead on the
                  look-ahead engines: BT pairs are swept in groups, census pairs run each pair's chain on its engine's stream)

The BT figures are the yardstick: the same process, the same clocks, the kernels of the commit before this option.  Every GPU step
(a warm-up pass, a timed pass, the stage calls of a cost) runs under a time limit of its own: a step that overruns ends the
process with status 124 and nothing further is started.  Prints one JSON line.  Needs a GPU: there is no fallback.  Reads nothing
but the package (the synthetic corridor).

    python tools/bench_sgbm_cost.py [--pairs 120] [--rounds 3] [--stage-calls 30] [--step-timeout 120]"""
import argparse
import json
import os
import signal
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=120, help="pairs per timed pass")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per cost, after one warm-up pass")
ap.add_argument("--stage-calls", type=int, default=30, help="timed synchronous pairs per cost and round for the stage brackets")
ap.add_argument("--step-timeout", type=int, default=120, help="seconds a single GPU step may take")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer, _native   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

SCHED = {_native.SCHED_DIAG: "diag", _native.SCHED_DIAG_RAGGED: "diag_ragged", _native.SCHED_UNFUSED: "unfused",
         _native.SCHED_VERT: "vert", _native.SCHED_VERT_RAGGED: "vert_ragged"}


def _overrun(signum, frame):
    sys.stderr.write("bench_sgbm_cost: a GPU step ran past its %d s: stopping, nothing further is started\n" % args.step_timeout)
    sys.stderr.flush()
    os._exit(124)


signal.signal(signal.SIGALRM, _overrun)


def step(fn, *a):
    """one GPU step under its own time limit"""
    signal.alarm(args.step_timeout)
    try:
        return fn(*a)
    finally:
        signal.alarm(0)


c = Corridor("C2")
frames = c.pairs(0, 48)
COSTS = {"bt": c.sgbm_params(), "census": c.sgbm_params(cost=1)}
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), COSTS["bt"], (c.w, c.h), max_keypoints=500)
ctx = cam._ctx
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]


def set_cost(params):
    cam.reset_lookahead()
    ctx.set_sgbm(params)
    cam.stereoSGBM.params = dict(params)
    cam.stereoSGBM.cost = int(params.get("cost", 0))


def compute_pass(params):
    set_cost(params)
    ctx.synchronize()
    t0 = time.perf_counter()
    for L, R in stream:
        cam.compute_3d(L, R, preprocessed=True)
    ctx.synchronize()
    return len(stream) / (time.perf_counter() - t0), SCHED[ctx.sgbm_last_schedule()]


def run_pass(params):
    set_cost(params)
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True)
    ctx.synchronize()
    accepted = 0
    t0 = time.perf_counter()
    for ok in odo.run(iter(stream)):
        accepted += bool(ok)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    return len(stream) / dt, accepted


def stage_pass(params):
    set_cost(params)
    names = ("sgbm_cost", "sgbm_agg", "sgbm_wta", "sgbm_post")
    rows = {k: [] for k in names}
    for i in range(-5, args.stage_calls):
        ctx.enable_timing(i >= 0, names)
        cam.compute_3d(*stream[i % len(stream)], preprocessed=True)
        ctx.synchronize()
        if i >= 0:
            t = ctx.timings(reset=True)
            for k in names:
                rows[k].append(t[k][0])
    ctx.enable_timing(False)
    return {k: {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4)}
            for k, v in rows.items()}


def alternate(one_pass):
    for params in COSTS.values():
        step(one_pass, params)                         # warm-up: allocations, clocks
    out = {k: [] for k in COSTS}
    for r in range(args.rounds):                       # the costs alternate inside every round
        for k, params in COSTS.items():
            out[k].append(step(one_pass, params))
    return out


result = {"tool": "bench_sgbm_cost", "device": ctx.device_name(), "rounds": args.rounds,
          "workload": "C2 1280x720, D = 128, mode 0, %d host pairs per pass (synthetic corridor, one GPU); census 9 x 7, P1 50, P2 200" % len(stream)}
stages = alternate(stage_pass)
result["stages_ms_per_round"] = stages
result["front_ms_median_per_round"] = {k: [r["sgbm_cost"]["median"] for r in v] for k, v in stages.items()}
result["front_census_over_bt_per_round"] = [round(a["sgbm_cost"]["median"] / b["sgbm_cost"]["median"], 3) for a, b in zip(stages["census"], stages["bt"])]
rates = alternate(compute_pass)
result["compute_3d_pairs_per_s"] = {k: {"per_round": [round(x[0], 1) for x in v], "median": round(float(np.median([x[0] for x in v])), 1),
                                        "schedule": v[0][1]} for k, v in rates.items()}
result["compute_3d_census_over_bt_per_round"] = [round(a[0] / b[0], 3) for a, b in zip(rates["census"], rates["bt"])]
runs = alternate(run_pass)
result["run_frames_per_s"] = {k: {"per_round": [round(x[0], 1) for x in v], "median": round(float(np.median([x[0] for x in v])), 1),
                                  "accepted": [x[1] for x in v]} for k, v in runs.items()}
result["run_census_over_bt_per_round"] = [round(a[0] / b[0], 3) for a, b in zip(runs["census"], runs["bt"])]
set_cost(COSTS["bt"])
ctx.close()
print(json.dumps(result))
