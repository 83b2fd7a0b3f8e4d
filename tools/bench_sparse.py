"""depth="sparse" beside depth="dense": wall time of one synchronous StereoOdometer.update() per pair over a C2 stream (1280x720,
D = 128, 500 features, host pairs), for pose_method="pnp" and the clique + outlier Umeyama odometer, and of vo_sparse_stereo alone
on a resident pair (microseconds; the library's event timers give its ORB and association + refinement + compaction parts).
Prints one JSON line.  Needs a GPU: there is no fallback.

    python tools/bench_sparse.py [--pairs N] [--rounds R] [--steps S]
    python tools/bench_sparse.py --run [--pairs 480] [--rounds 3] [--engines N] [--host]

update() is the synchronous entry: nothing is submitted ahead in either mode, so the dense figure of the first form is NOT the
throughput of run() with its look-ahead engines (bench.py measures that).

--run: the streamed rates instead.  Pairs per second of StereoOdometer.run() over C2 host pairs in dense and in sparse mode, and of the
plain update() loop in sparse mode (what run() did in that mode before sparse pairs were submitted ahead: the same-process baseline),
for pose_method="pnp" and the clique + outlier Umeyama odometer; one warm-up pass, then --rounds timed passes per mode, the modes
alternating.  --engines N: the context's look-ahead engines (default: the library's).  --host: one more sparse run() pass per pose
method with every native call of the driving thread timed -- per pair the time inside calls that WAIT for the GPU (collecting a
pair, ending a pose step, a staging copy) and inside calls that only enqueue; the rest of the wall time is the interpreter.  A loop
whose waiting share is near zero is bound by the host thread (a binding that calls another one, pnp_pair_begin_window ->
pnp_pair_begin, is counted under both names).  Exit status 1 when the sparse run() rate is not above the update() loop's in some round."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=None, help="pairs per timed pass (default 48; 480 with --run)")
ap.add_argument("--run", action="store_true", help="the streamed rates: run() dense / sparse and the sparse update() loop")
ap.add_argument("--engines", type=int, default=None, help="--run: look-ahead engines of the context")
ap.add_argument("--host", action="store_true", help="--run: time the driving thread's native calls in one more sparse run() pass")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per mode, after one warm-up pass")
ap.add_argument("--steps", type=int, default=200, help="timed vo_sparse_stereo calls")
ap.add_argument("--assoc", action="store_true", help="--run: the sparse legs with sparse_mutual=True, sparse_ratio=0.8, loop_check=48")
ap.add_argument("--tag", default=None, help="--run: a label for the result line")
args = ap.parse_args()
if args.pairs is None:
    args.pairs = 480 if args.run else 48
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500,
                   engines=args.engines if args.run else None)
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


WAITS = ("sparse_stereo", "pose_pair_end", "pnp_pair_end", "host_stage_wait", "synchronize", "orb_slot_count")


def stream_pass(kw, how):
    """-> (pairs per second, accepted frames) of one pass over the stream through run() or the plain update() loop"""
    odo = StereoOdometer(cam, nfeatures=500, preprocessed_frames=True, **kw)
    ctx.synchronize()
    t0 = time.perf_counter()
    if how == "run":
        accepted = sum(bool(ok) for ok in odo.run(iter(stream)))
    else:
        accepted = sum(bool(odo.update(L, R)) for L, R in stream)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    return len(stream) / dt, accepted


def host_pass(kw):
    """one sparse run() pass with the driving thread's native calls timed (the two calls the odometer treats as seams when replaced
    stay as they are: the fused pose step must keep running)"""
    T = {}

    def wrap(name):
        f = getattr(ctx, name)

        def g(*a, **k):
            t0 = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                T[name] = T.get(name, 0.0) + time.perf_counter() - t0
        setattr(ctx, name, g)
    names = [n for n in dir(ctx) if not n.startswith("_") and callable(getattr(ctx, n)) and n not in ("close", "point_clouds", "ransac_pnp")]
    for n in names:
        wrap(n)
    try:
        rate, _ = stream_pass(kw, "run")
    finally:
        for n in names:
            delattr(ctx, n)
    us = 1e6 / len(stream)
    wait = sum(v for k, v in T.items() if k in WAITS)
    return {"pairs_per_s": round(rate, 1), "wall_us_per_pair": round(1e6 / rate, 1), "native_wait_us_per_pair": round(wait * us, 1),
            "native_enqueue_us_per_pair": round((sum(T.values()) - wait) * us, 1),
            "top_calls_us_per_pair": {k: round(v * us, 1) for k, v in sorted(T.items(), key=lambda kv: -kv[1])[:6]}}


if args.run:
    LEGS = {"run_dense": ("dense", "run"), "run_sparse": ("sparse", "run"), "update_sparse": ("sparse", "update")}
    ON = dict(sparse_mutual=True, sparse_ratio=0.8, loop_check=48) if args.assoc else {}

    def leg_kw(d, pkw):
        return dict(depth=d, **pkw, **(ON if d == "sparse" else {}))
    result = {"tool": "bench_sparse --run", "workload": "C2 1280x720 D=128, 500 features, %d host pairs per pass (synthetic corridor, one GPU)" % len(stream),
              "device": ctx.device_name(), "engines": ctx.set_engines(0), "rounds": args.rounds, "library": os.path.basename(os.environ.get("VO355_LIB", "libvo355.so")),
              "sparse_options": {k: v for k, v in ON.items()}, "tag": args.tag, "pairs_per_s": {}}
    for p, pkw in POSE.items():
        for leg, (d, how) in LEGS.items():
            stream_pass(leg_kw(d, pkw), how)           # warm-up: allocations (an engine's scratch comes with its first pair), clocks
    rates = {"%s_%s" % (leg, p): [] for p in POSE for leg in LEGS}
    for r in range(args.rounds):                       # the modes alternate inside every round
        for p, pkw in POSE.items():
            for leg, (d, how) in LEGS.items():
                rates["%s_%s" % (leg, p)].append(stream_pass(leg_kw(d, pkw), how))
    for k, v in rates.items():
        result["pairs_per_s"][k] = {"per_round": [round(x, 1) for x, _ in v], "median": round(float(np.median([x for x, _ in v])), 1),
                                    "accepted": [a for _, a in v]}
    for p in POSE:
        result["pairs_per_s"]["run_over_update_sparse_%s" % p] = round(min(a / b for (a, _), (b, _) in zip(rates["run_sparse_" + p], rates["update_sparse_" + p])), 3)
    # the feature: run() in sparse mode must beat the update() loop in every round of every invocation (exit status 1 otherwise)
    result["run_sparse_above_update_sparse"] = all(result["pairs_per_s"]["run_over_update_sparse_%s" % p] > 1.0 for p in POSE)
    if args.host:
        result["host"] = {p: host_pass(leg_kw("sparse", pkw)) for p, pkw in POSE.items()}
    print(json.dumps(result))
    sys.exit(0 if result["run_sparse_above_update_sparse"] else 1)

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
