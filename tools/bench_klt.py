"""match="klt" and match="klt" with klt_fused=True beside match="orb": frames per second of synchronous StereoOdometer.update()
loops and of StereoOdometer.run() (pairs submitted ahead, pose steps begun ahead) over a C2 stream (1280x720, 500 features, dense
depth, pose_method="pnp", host pairs), the three modes alternating inside every round of ONE process; the synchronous pair step
alone (the median of --step-calls klt_pnp_pair calls against the three composed calls klt_track -> points3d_at -> ransac_pnp on
the same two slots, 500 keypoints); and the two Lucas-Kanade kernels alone at 500 and 8000 points on a 1280x720 pair (the library's event brackets: the pyramid launches under
"orb", the forward and backward tracking launches under "match"; median of --steps calls after 10 warm-up calls).  Prints one JSON
line.  Needs a GPU: there is no fallback.  Reads nothing but the package (the synthetic corridor).

    python tools/bench_klt.py [--pairs 240] [--rounds 3] [--steps 50] [--step-calls 200]"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=240, help="pairs per timed pass")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per mode, after one warm-up pass")
ap.add_argument("--steps", type=int, default=50, help="timed tracking calls per point count")
ap.add_argument("--step-calls", type=int, default=200, help="timed calls of the pair step, fused and composed")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import StereoCamera, StereoOdometer, _native   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
frames = c.pairs(0, 48)
result = {"tool": "bench_klt", "kernels_us": {}}

# ---------------------------------------------------------------------------------------------- the two kernels alone
ctx = _native.Context(0, c.w, c.h, 128, 4000)          # kp_cap 9024
result["device"] = ctx.device_name()
a, b = frames[0][0], frames[1][0]
rng = np.random.default_rng(5)
for n in (500, 8000):
    xy = np.stack([rng.uniform(30, c.w - 31, n), rng.uniform(30, c.h - 31, n)], 1).astype(np.float32)
    rows = {"pyramids": [], "tracking_forward_and_backward": []}
    kept = its = 0
    for step in range(-10, args.steps):
        ctx.enable_timing(step >= 0)
        _, st, it = ctx.klt_track_host(a, b, xy)
        if step < 0:
            continue
        t = ctx.timings(reset=True)
        rows["pyramids"].append(1e3 * t["orb"][0])
        rows["tracking_forward_and_backward"].append(1e3 * t["match"][0])
        kept, its = int((st == 0).sum()), float(it.mean())
    ctx.enable_timing(False)
    result["kernels_us"][str(n)] = dict(kept=kept, mean_iterations=round(its, 1),
                                        **{k: {"median": round(float(np.median(v)), 1), "p10": round(float(np.percentile(v, 10)), 1),
                                               "p90": round(float(np.percentile(v, 90)), 1)} for k, v in rows.items()})
ctx.close()

# ---------------------------------------------------------------------------------------------- the update() loops
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
ctx = cam._ctx
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]
BASE = dict(nfeatures=500, preprocessed_frames=True, pose_method="pnp")
MODES = {"orb": dict(), "klt": dict(match="klt"), "klt_fused": dict(match="klt", klt_fused=True)}


def one_pass(kw):
    odo = StereoOdometer(cam, **BASE, **kw)
    ctx.synchronize()
    accepted = 0
    t0 = time.perf_counter()
    for L, R in stream:
        accepted += bool(odo.update(L, R))
    ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    return len(stream) / dt, accepted


def one_run(kw):
    odo = StereoOdometer(cam, **BASE, **kw)
    ctx.synchronize()
    accepted = 0
    t0 = time.perf_counter()
    for ok in odo.run(iter(stream)):
        accepted += bool(ok)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    ahead = getattr(odo, "klt_ahead", None)
    odo.reset_lookahead()
    return len(stream) / dt, accepted, ahead


def report(rates):
    out = {k: {"per_round": [round(x[0], 1) for x in v], "median": round(float(np.median([x[0] for x in v])), 1),
               "accepted": [x[1] for x in v]} for k, v in rates.items()}
    for k, v in rates.items():
        if len(v[0]) > 2 and v[0][2] is not None:
            out[k]["begun_ahead"] = [x[2] for x in v]
    return out


def pair_step():
    """the synchronous pair step alone on two slots of the stream: one fused call against the three composed calls"""
    x3, disp, left = cam.compute_3d(*stream[0], preprocessed=True)
    probe = StereoOdometer(cam, **BASE)
    kps, _ = probe.orb.detectAndCompute(left, probe.feature_mask(disp))
    x3b, _, _ = cam.compute_3d(*stream[1], preprocessed=True)
    sa, sb, xy = x3.frame.slot, x3b.frame.slot, kps.xy
    Q = cam.Q
    K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
    roi0 = np.array(x3b.frame.roi[:2], np.float32)

    def fused():
        return ctx.klt_pnp_pair(sa, sb, K4, win=21, levels=4, fb=1.0)["best_count"]

    def composed():
        xy_b, st, _ = ctx.klt_track(sa, sb, win=21, levels=4, fb=1.0)
        idx = np.nonzero(st == 0)[0]
        pts, st_a = ctx.points3d_at(sa, xy[idx])
        ok = (st_a == 0) & np.isfinite(pts).all(axis=1)
        return ctx.ransac_pnp(pts[ok], xy_b[idx[ok]] + roi0, K4, 256, 1.5, 4321)["best_count"]

    out = {"keypoints": len(xy)}
    times = {"fused": [], "composed": []}
    for step in range(-10, args.step_calls):
        for name, fn in (("fused", fused), ("composed", composed)):       # alternating call by call
            t0 = time.perf_counter()
            out["best_count_" + name] = int(fn())
            if step >= 0:
                times[name].append(1e6 * (time.perf_counter() - t0))
    for name, v in times.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 1), "p10": round(float(np.percentile(v, 10)), 1), "p90": round(float(np.percentile(v, 90)), 1)}
    return out


result["workload"] = ("C2 1280x720, 500 features, dense depth, pose_method=pnp, %d host pairs per pass through synchronous "
                      "StereoOdometer.update() (synthetic corridor, one GPU)" % len(stream))
result["rounds"] = args.rounds
for kw in MODES.values():
    one_pass(kw)                                       # warm-up: allocations, clocks
rates = {k: [] for k in MODES}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, kw in MODES.items():
        rates[k].append(one_pass(kw))
result["frames_per_s"] = report(rates)
result["klt_over_orb_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(rates["klt"], rates["orb"])]
result["klt_fused_over_orb_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(rates["klt_fused"], rates["orb"])]
result["klt_fused_over_klt_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(rates["klt_fused"], rates["klt"])]
# ---------------------------------------------------------------------------------------------- the run() loops
for kw in MODES.values():
    one_run(kw)
runs = {k: [] for k in MODES}
for r in range(args.rounds):
    for k, kw in MODES.items():
        runs[k].append(one_run(kw))
result["run_frames_per_s"] = report(runs)
result["run_klt_over_orb_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(runs["klt"], runs["orb"])]
result["run_klt_fused_over_orb_per_round"] = [round(a_[0] / b_[0], 3) for a_, b_ in zip(runs["klt_fused"], runs["orb"])]
# ---------------------------------------------------------------------------------------------- the pair step alone
result["pair_step"] = pair_step()
ctx.close()
print(json.dumps(result))
