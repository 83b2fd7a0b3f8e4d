"""pose_method="pnp" beside the default: pairs/s of StereoOdometer.run() over a C2 stream (1280x720, D = 128, 500 features, host
pairs, default look-ahead) and the wall time of one synchronous pair step on two resident frames, for pnp_refine 0 and 3 and for
pose_method="umeyama", and for pnp_refine 3 with --lo-rounds local-optimisation rounds (pnp_lo_rounds; default 3, 0 leaves the mode
out).  The modes alternate in one process: run() by run(), and the synchronous steps one by one.  Prints one JSON line.  Needs a
GPU: there is no fallback.

    python tools/bench_pnp.py [--pairs N] [--rounds R] [--steps S] [--lo-rounds K] [--tree DIR]

--tree DIR measures another checkout of the project (an A/B against an older commit: a tree whose StereoOdometer has no pnp_refine
reports null for that mode and "fused": false; one without pnp_lo_rounds reports null for the rounds)."""
import argparse
import inspect
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=96, help="pairs per timed run() (the 48 rendered frames forwards, backwards, ...)")
ap.add_argument("--rounds", type=int, default=3, help="timed run()s per mode, after one warm-up run")
ap.add_argument("--steps", type=int, default=300, help="timed synchronous pair steps per mode")
ap.add_argument("--lo-rounds", type=int, default=3, help="pnp_lo_rounds of the mode pnp_refine_3_lo (0: no such mode)")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
frames = c.pairs(0, 48)
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]
has_refine = "pnp_refine" in inspect.signature(StereoOdometer.__init__).parameters
has_lo = "pnp_lo_rounds" in inspect.signature(StereoOdometer.__init__).parameters
MODES = {"pnp_refine_0": dict(pose_method="pnp"), "pnp_refine_3": dict(pose_method="pnp", pnp_refine=3),
         "umeyama": dict(rigidity_threshold=0.1, outlier_threshold=0.02)}
if args.lo_rounds > 0:
    MODES["pnp_refine_3_lo"] = dict(pose_method="pnp", pnp_refine=3, pnp_lo_rounds=args.lo_rounds)


def make(kw):
    return StereoOdometer(cam, nfeatures=500, preprocessed_frames=True, **kw)


def run_rate(kw):
    odo = make(kw)
    cam._ctx.synchronize()
    t0 = time.perf_counter()
    accepted = sum(bool(ok) for ok in odo.run(iter(stream)))
    cam._ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    return len(stream) / dt, accepted


def step_times(modes):
    """one synchronous pair step (matching + pose of two resident frames, nothing begun ahead) per mode, the modes taking turns
    step by step -> {mode: microseconds}"""
    odos = {}
    for k, kw in modes.items():
        odo = make(kw)
        assert odo.update(*frames[0]) and odo.update(*frames[1])
        odo.reset_lookahead()
        odos[k] = (odo, (odo.prev_kps, odo.prev_desc, odo.prev_3d), (odo.current_kps, odo.current_desc, odo.current_3d))
    out = {k: [] for k in modes}
    for _ in range(args.steps + 20):
        for k, (odo, a, b) in odos.items():
            t0 = time.perf_counter()
            T = odo._try_pair(*a, *b)
            out[k].append(1e6 * (time.perf_counter() - t0))
            assert T is not None
    return {k: np.array(v[20:]) for k, v in out.items()}


result = {"tool": "bench_pnp", "workload": "C2 1280x720 D=128, 500 features, host pairs through StereoOdometer.run()",
          "device": cam._ctx.device_name(), "pairs": len(stream), "rounds": args.rounds, "steps": args.steps, "lo_rounds": args.lo_rounds,
          "fused": bool(getattr(StereoOdometer, "_pnp_fused", False)), "modes": {}}
live = {k: v for k, v in MODES.items() if (has_refine or "pnp_refine" not in v) and (has_lo or "pnp_lo_rounds" not in v)}
for kw in live.values():
    run_rate(kw)                                       # warm-up: allocations, clocks, every alternate built
rates = {k: [] for k in live}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, kw in live.items():
        rates[k].append(run_rate(kw))
steps = step_times(live)
for k in MODES:
    if k not in live:
        result["modes"][k] = None
        continue
    st = steps[k]
    rr = [x[0] for x in rates[k]]
    result["modes"][k] = {"pairs_per_s": [round(x, 1) for x in rr], "pairs_per_s_mean": round(float(np.mean(rr)), 1),
                          "accepted": [x[1] for x in rates[k]], "step_us_median": round(float(np.median(st)), 1),
                          "step_us_p10": round(float(np.percentile(st, 10)), 1), "step_us_p90": round(float(np.percentile(st, 90)), 1)}
print(json.dumps(result))
