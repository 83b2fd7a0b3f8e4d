"""MonoOdometer with the pose recovered on the device beside today's mode: pairs/s of update() over a staged C5 stream (1920x1080,
8000 keypoints, 5000 hypotheses, five-point solver, default look-ahead and speculation) for the three modes -- "host" (today's:
140 KB record, cheirality vote on a worker thread), "device" (pose_on_device) and "device_scale" (+ propagate_scale) -- alternating
inside one process on one context.  Per mode: pairs/s of every timed run, the host milliseconds per frame spent inside native calls
(wall timers around the context's methods, as tools/mono_host.py counts them: calls that only enqueue, and calls that wait for the
device -- the _end of a pair step, a keypoint count) and the bytes a pair step writes into its pinned record.  Prints one JSON line.  Needs a GPU: there is no fallback.

    python tools/bench_mono_pose.py [--frames N] [--warmup W] [--rounds R]"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120, help="frames per timed run (after the warm-up frames)")
ap.add_argument("--warmup", type=int, default=12, help="frames in front of the clock in every run")
ap.add_argument("--rounds", type=int, default=3, help="timed runs per mode, after one warm-up run")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import _native                        # noqa: E402
from openvo_amd.mono import MonoOdometer              # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C5")
K = np.array([[c.f, 0, c.cx], [0, c.f, c.cy], [0, 0, 1.0]])
n_img = args.warmup + args.frames
frames = [p[0] for p in c.pairs(0, n_img)]
ctx = _native.Context(0, c.w, c.h, 16, 8000)
MODES = {"host": {}, "device": dict(pose_on_device=True), "device_scale": dict(pose_on_device=True, propagate_scale=True)}

native_s = [0.0, 0.0]                                  # seconds inside native calls since the last reset: enqueue-only, waiting
WAITS = ("mono_pair_end", "mono_pose_pair_end", "orb_slot_count", "download_keypoints_xy")


def wrap(name):
    f, slot = getattr(ctx, name), int(name in WAITS)

    def g(*a, **k):
        t0 = time.perf_counter()
        r = f(*a, **k)
        native_s[slot] += time.perf_counter() - t0
        return r
    setattr(ctx, name, g)


for name in dir(ctx):
    if not name.startswith("_") and callable(getattr(ctx, name)) and name not in ("close", "synchronize"):
        wrap(name)

odos = {k: MonoOdometer(K, (c.w, c.h), nfeatures=8000, ransac_iters=5000, solver=5, context=ctx, **kw) for k, kw in MODES.items()}
next(iter(odos.values())).stage_frames(frames)
for o in odos.values():
    o._n_staged = n_img                                # (one context, one staged stream: every odometer reads it)


def run(odo):
    """-> pairs/s, native ms per frame (enqueue-only calls, waiting calls), accepted frames, bytes of the last pair's record"""
    odo.restart()                                      # the odometers take turns on the context's slots: nothing of the last run is kept
    for k in range(args.warmup):
        odo.update(k)
    odo.reset_lookahead()                              # nothing computed before the clock starts is used after it
    ctx.synchronize()
    gc.collect()
    gc.disable()
    native_s[0] = native_s[1] = 0.0
    acc = 0
    t0 = time.perf_counter()
    for k in range(args.warmup, n_img):
        acc += bool(odo.update(k))
    pose = odo.c_T_w                                   # (the host mode's pending pose recoveries are part of its work)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    if odo.pose_on_device:
        rec = ctypes.sizeof(_native.MonoPose)
    else:                                              # header + E, then mask / q / t of the first frame's keypoints and xy of the second's
        nb = ctx.orb_slot_count(odo._ref[0], 8000, 0)
        rec = 64 + 72 + 9 * nb + 8 * nb                # (consecutive frames hold the same number of keypoints to within a few)
    assert np.isfinite(pose).all()
    return args.frames / dt, (1e3 * native_s[0] / args.frames, 1e3 * native_s[1] / args.frames), acc, rec


for o in odos.values():
    run(o)                                             # warm-up: allocations, clocks, every alternate built
res = {k: [] for k in MODES}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, o in odos.items():
        res[k].append(run(o))
out = {"tool": "bench_mono_pose", "workload": "C5 1920x1080, 8000 keypoints, 5000 hypotheses, five-point solver, staged frames",
       "device": ctx.device_name(), "frames": args.frames, "warmup": args.warmup, "rounds": args.rounds,
       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "modes": {}}
for k, rr in res.items():
    rate = [x[0] for x in rr]
    out["modes"][k] = {"pairs_per_s": [round(x, 1) for x in rate], "pairs_per_s_mean": round(float(np.mean(rate)), 1),
                       "pairs_per_s_range": [round(min(rate), 1), round(max(rate), 1)],
                       "native_enqueue_ms_per_frame": [round(x[1][0], 4) for x in rr],
                       "native_wait_ms_per_frame": [round(x[1][1], 4) for x in rr], "accepted": [x[2] for x in rr],
                       "record_bytes_per_pair": rr[-1][3], "scale": round(float(odos[k].scale), 4), "scale_status": odos[k].scale_status}
for o in odos.values():
    o.close()
ctx.close()
print(json.dumps(out))
