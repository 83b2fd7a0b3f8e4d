"""pose_method="pnp" beside the default: pairs/s of StereoOdometer.run() over a C2 stream (1280x720, D = 128, 500 features, host
pairs, default look-ahead) and the wall time of one synchronous pair step on two resident frames, for pnp_refine 0 and 3 and for
pose_method="umeyama".  Prints one JSON line.  Needs a GPU: there is no fallback.

    python tools/bench_pnp.py [--pairs N] [--rounds R] [--steps S] [--tree DIR]

--tree DIR measures another checkout of the project (an A/B against an older commit: a tree whose StereoOdometer has no pnp_refine
reports null for that mode and "fused": false)."""
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
MODES = {"pnp_refine_0": dict(pose_method="pnp"), "pnp_refine_3": dict(pose_method="pnp", pnp_refine=3),
         "umeyama": dict(rigidity_threshold=0.1, outlier_threshold=0.02)}


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


def step_times(kw):
    """one synchronous pair step (matching + pose of two resident frames, nothing begun ahead), microseconds"""
    odo = make(kw)
    assert odo.update(*frames[0]) and odo.update(*frames[1])
    odo.reset_lookahead()
    a = (odo.prev_kps, odo.prev_desc, odo.prev_3d)
    b = (odo.current_kps, odo.current_desc, odo.current_3d)
    out = []
    for k in range(args.steps + 20):
        t0 = time.perf_counter()
        T = odo._try_pair(*a, *b)
        out.append(1e6 * (time.perf_counter() - t0))
        assert T is not None
    return np.array(out[20:])


result = {"tool": "bench_pnp", "workload": "C2 1280x720 D=128, 500 features, host pairs through StereoOdometer.run()",
          "device": cam._ctx.device_name(), "pairs": len(stream), "rounds": args.rounds, "steps": args.steps,
          "fused": bool(getattr(StereoOdometer, "_pnp_fused", False)), "modes": {}}
live = {k: v for k, v in MODES.items() if has_refine or "pnp_refine" not in v}
for kw in live.values():
    run_rate(kw)                                       # warm-up: allocations, clocks, every alternate built
rates = {k: [] for k in live}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, kw in live.items():
        rates[k].append(run_rate(kw))
for k in MODES:
    if k not in live:
        result["modes"][k] = None
        continue
    st = step_times(live[k])
    rr = [x[0] for x in rates[k]]
    result["modes"][k] = {"pairs_per_s": [round(x, 1) for x in rr], "pairs_per_s_mean": round(float(np.mean(rr)), 1),
                          "accepted": [x[1] for x in rates[k]], "step_us_median": round(float(np.median(st)), 1),
                          "step_us_p10": round(float(np.percentile(st, 10)), 1), "step_us_p90": round(float(np.percentile(st, 90)), 1)}
print(json.dumps(result))
