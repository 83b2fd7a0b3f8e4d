"""depth="sparse" beside depth="dense": wall time of one synchronous StereoOdometer.update() per pair over a C2 stream (1280x720,
D = 128, 500 features, host pairs), for pose_method="pnp" and the clique + outlier Umeyama odometer, and of vo_sparse_stereo alone
on a resident pair (microseconds; the library's event timers give its ORB and association + refinement + compaction parts).
Prints one JSON line.  Needs a GPU: there is no fallback.

    python tools/bench_sparse.py [--pairs N] [--rounds R] [--steps S]

update() is the synchronous entry: nothing is submitted ahead in either mode, so the dense figure is NOT the throughput of
run() with its look-ahead engines (bench.py measures that)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=48, help="pairs per timed pass through update()")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per mode, after one warm-up pass")
ap.add_argument("--steps", type=int, default=200, help="timed vo_sparse_stereo calls")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
ctx = cam._ctx
frames = c.pairs(0, 48)
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]
POSE = {"pnp": dict(pose_method="pnp"), "umeyama_clique": dict(rigidity_threshold=0.1, outlier_threshold=0.02)}
MODES = {"%s_%s" % (d, p): dict(depth=d, **kw) for p, kw in POSE.items() for d in ("dense", "sparse")}


def one_pass(kw):
    """-> (microseconds per update() call, accepted frames)"""
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True, **kw)
    ctx.synchronize()
    t, accepted = [], 0
    for L, R in stream:
        t0 = time.perf_counter()
        accepted += bool(odo.update(L, R))
        t.append(1e6 * (time.perf_counter() - t0))
    odo.reset_lookahead()
    return np.array(t[1:]), accepted                   # (the first call pairs nothing)


def sparse_alone():
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True, depth="sparse")
    slot = 0
    ctx.upload_pair(slot, *frames[0], True)
    counts = None
    for _ in range(20):
        counts = ctx.sparse_stereo(slot, 500, odo.MIN_VALID_DISPARITY, odo.MAX_VALID_DISPARITY, odo.sparse_row_tol, odo.sparse_max_hamming)
    ctx.enable_timing(True, stages=("orb", "match"))
    ctx.timings(reset=True)
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        ctx.sparse_stereo(slot, 500, odo.MIN_VALID_DISPARITY, odo.MAX_VALID_DISPARITY, odo.sparse_row_tol, odo.sparse_max_hamming)
        t.append(1e6 * (time.perf_counter() - t0))
    ev = ctx.timings(reset=True)
    ctx.enable_timing(False)
    t = np.array(t)
    return {"counts3": [int(v) for v in counts], "call_us_median": round(float(np.median(t)), 1), "call_us_p10": round(float(np.percentile(t, 10)), 1),
            "call_us_p90": round(float(np.percentile(t, 90)), 1),
            "orb_two_chains_us": round(1e3 * ev["orb"][0] / args.steps, 1), "match_refine_compact_us": round(1e3 * ev["match"][0] / args.steps, 1)}


result = {"tool": "bench_sparse", "workload": "C2 1280x720 D=128, 500 features, host pairs through synchronous StereoOdometer.update()",
          "device": ctx.device_name(), "pairs": len(stream), "rounds": args.rounds, "modes": {}}
for kw in MODES.values():
    one_pass(kw)                                       # warm-up: allocations, clocks
times = {k: [] for k in MODES}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, kw in MODES.items():
        times[k].append(one_pass(kw))
for k in MODES:
    med = [float(np.median(t)) for t, _ in times[k]]
    result["modes"][k] = {"update_us_median_per_round": [round(x, 1) for x in med], "update_us_median": round(float(np.median(med)), 1),
                          "accepted": [a for _, a in times[k]]}
result["vo_sparse_stereo"] = sparse_alone()
print(json.dumps(result))
