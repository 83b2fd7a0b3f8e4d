"""track="map" with and without map_fused beside pair mode: frames per second of synchronous StereoOdometer.update() loops over a C2
stream (1280x720, 500 features, depth="sparse", pose_method="pnp", host pairs), the three modes alternating inside every round of ONE
process; and the map step alone on planted maps of 1200 and 3800 landmarks -- the fused call (vo_track_map) against the three calls
of the unfused chain with the host's arithmetic between them (host clock around the calls, their synchronisations included), and
the library's event brackets of the three kernels the fused step adds, of the two it replaces, and of the kNN-2 launch, which the
fused step shapes for the map's size n and the unfused chain for the visible count.  Prints one JSON line.  Needs a GPU: there is
no fallback.  Reads nothing but the package (the synthetic corridor and seeded random maps).

    python tools/bench_map.py [--pairs 960] [--rounds 3] [--steps 200]

The planted maps need the test-only build of the library (planting is not a product entry): that part runs in a child process
with VO355_LIB pointing at openvo_amd/libvo355_hooks.so; --no-kernels leaves it out."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=960, help="pairs per timed pass")
ap.add_argument("--rounds", type=int, default=3, help="timed passes per mode, after one warm-up pass")
ap.add_argument("--steps", type=int, default=200, help="timed map steps per map size")
ap.add_argument("--no-kernels", action="store_true", help="leave out the planted-map part")
ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np                                    # noqa: E402
from openvo_amd import _native                        # noqa: E402

W, H = 1280, 720
K4 = (700.0, 700.0, 640.0, 360.0)
RATIO, ITERS, THR, SEED = 0.8, 256, 1.5, 4321


# ---------------------------------------------------------------------------------------------- the map step alone (child process)
def _scene(n, nk, n_match, rng):
    """n landmarks, nine in ten inside the image under the identity pose; a frame of nk keypoints of which n_match see a visible
    landmark again from a camera moved by 5 cm and 0.02 rad"""
    z = rng.uniform(2.0, 20.0, n)
    u, v = rng.uniform(5, W - 6, n), rng.uniform(5, H - 6, n)
    out = rng.random(n) < 0.1
    u[out] += 2 * W
    xyz = np.stack([(u - K4[2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z], 1).astype(np.float32)
    desc, rdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    m = dict(xyz=xyz, desc=desc, rdesc=rdesc, octave=np.zeros(n, np.int32), obs=np.ones(n, np.int32), last=np.zeros(n, np.int32))
    a = 0.02
    R, t = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), np.array([0.02, 0.0, 0.05])
    q = rng.choice(np.flatnonzero(~out), n_match, replace=False)
    f = dict(xy=np.stack([rng.uniform(0, W, nk), rng.uniform(0, H, nk)], 1), desc=rng.integers(0, 256, (nk, 32), dtype=np.uint8),
             xyz=np.stack([rng.uniform(-3, 3, nk), rng.uniform(-2, 2, nk), rng.uniform(2, 20, nk)], 1), rdesc=rng.integers(0, 256, (nk, 32), dtype=np.uint8))
    Y = xyz[q].astype(np.float64) @ R.T + t
    f["xyz"][:n_match] = Y
    f["xy"][:n_match] = np.stack([K4[0] * Y[:, 0] / Y[:, 2] + K4[2], K4[1] * Y[:, 1] / Y[:, 2] + K4[3]], 1) + rng.normal(0, 0.3, (n_match, 2))
    f["desc"][:n_match] = desc[q]
    return m, {k: np.ascontiguousarray(v, np.uint8 if "desc" in k else np.float32) for k, v in f.items()}


def _brackets(ctx):
    """the event brackets of the calls since the last look, by stage, in the order they were opened -> {stage: [microseconds]}"""
    out = {}
    for stage, _, b, e in ctx.stage_timeline():
        out.setdefault(stage, []).append(1e3 * (e - b))
    ctx.timings(reset=True)
    return out


def kernels_child():
    ctx = _native.Context(0, W, H, 128, 2000)             # kp_cap 5024
    Q = np.eye(4)
    Q[3, 3] = 0.0; Q[2, 3] = K4[0]; Q[0, 3] = -K4[2]; Q[1, 3] = -K4[3]; Q[3, 2] = 10.0
    ctx.set_Q(Q)
    blank = np.zeros((H, W), np.uint8)
    NEW, VIEW = 5, 3
    ctx.upload_pair(NEW, blank, blank, True)
    I34 = np.eye(4)[:3]
    res = {}
    for n in (1200, 3800):
        rng = np.random.default_rng(n)
        m, f = _scene(n, 500, 300, rng)
        h = ctx.map_create(5024)
        ctx.plant_keypoints(NEW, f["xy"], f["desc"], f["xyz"], f["rdesc"])
        rows = {k: [] for k in ("fused_call", "unfused_calls", "k_map_view_pad", "k_map_decide", "k_map_update_dev", "knn_fused", "pnp_chain_fused",
                                "k_map_view", "k_map_update", "knn_unfused", "pnp_chain_unfused")}
        fig = {}
        for step in range(-20, args.steps):                # 20 of each as warm-up, then alternating
            ctx.enable_timing(step >= 0)
            for kind in ("fused", "unfused"):
                ctx.plant_map(h, **m)                      # (the map is what it was: planting is outside every clock)
                ctx.synchronize()
                t0 = time.perf_counter()
                if kind == "fused":
                    r = ctx.map_track(h, NEW, VIEW, I34, K4, 0.1, RATIO, ITERS, THR, SEED, 0, 10, 1.0, np.pi / 3, 1, 5, 8, want_matches=False)
                    ok = r["decision"] == 0
                    fig = dict(visible=int(r["view"][1]), matches=r["matches"], inliers=r["best_count"], size_after=int(r["update"][5]))
                else:
                    c2 = ctx.map_view(h, I34, K4, 0.1, NEW, VIEW)
                    r = ctx.pnp_pair(VIEW, NEW, RATIO, K4, ITERS, THR, SEED, 0, True)
                    T = np.vstack([r["Rt"], [0, 0, 0, 1]])
                    ok = r["matches"] >= 10 and r["n"] >= 10 and r["best_count"] >= 10 and not np.isnan(T).any() and \
                        np.linalg.norm(T[:3, 3]) <= 1.0 and np.linalg.norm(ctx.rodrigues(T[:3, :3])) <= np.pi / 3 and c2[1] >= 10
                    ctx.map_update(h, NEW, np.linalg.inv(T @ np.eye(4)), 1, 5, 8, r["q"], r["t"], r["mask"])
                dt = 1e6 * (time.perf_counter() - t0)
                assert ok, "the planted step was not accepted"
                if step < 0:
                    continue
                b = _brackets(ctx)
                if kind == "fused":
                    rows["fused_call"].append(dt)
                    for k, v in (("k_map_view_pad", b["match"][0]), ("knn_fused", b["knn"][0]), ("pnp_chain_fused", b["pose"][0]),
                                 ("k_map_decide", b["pose"][1]), ("k_map_update_dev", b["pose"][2])):
                        rows[k].append(v)
                else:
                    rows["unfused_calls"].append(dt)
                    for k, v in (("k_map_view", b["match"][0]), ("knn_unfused", b["knn"][0]), ("pnp_chain_unfused", b["pose"][0]), ("k_map_update", b["pose"][1])):
                        rows[k].append(v)
        ctx.enable_timing(False)
        ctx.map_destroy(h)
        res[str(n)] = dict(fig, us={k: {"median": round(float(np.median(v)), 1), "p10": round(float(np.percentile(v, 10)), 1),
                                        "p90": round(float(np.percentile(v, 90)), 1)} for k, v in rows.items()})
    ctx.close()
    print("KERNELS " + json.dumps(res))


if args.kernels_child:
    kernels_child()
    sys.exit(0)

# ---------------------------------------------------------------------------------------------- the update() loops
from openvo_amd import StereoCamera, StereoOdometer   # noqa: E402
from openvo_amd.synth import Corridor                 # noqa: E402

c = Corridor("C2")
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
ctx = cam._ctx
frames = c.pairs(0, 48)
order = list(range(48)) + list(range(46, 0, -1))       # there and back: every step is a small motion
stream = [frames[order[k % len(order)]] for k in range(args.pairs)]
BASE = dict(nfeatures=500, preprocessed_frames=True, depth="sparse", pose_method="pnp")
MODES = {"pair": dict(), "map": dict(track="map"), "map_fused": dict(track="map", map_fused=True)}


def one_pass(kw):
    """-> (frames per second, accepted frames, frames the map step placed, largest map)"""
    odo = StereoOdometer(cam, **BASE, **kw)
    ctx.synchronize()
    accepted = by_map = largest = 0
    t0 = time.perf_counter()
    for L, R in stream:
        accepted += bool(odo.update(L, R))
        by_map += odo.track_source == "map"
        largest = max(largest, odo._map_size)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    odo.reset_lookahead()
    if kw:
        odo.release_map()
    return len(stream) / dt, accepted, by_map, largest


result = {"tool": "bench_map", "workload": "C2 1280x720, 500 features, depth=sparse, pose_method=pnp, %d host pairs per pass through synchronous "
          "StereoOdometer.update() (synthetic corridor, one GPU)" % len(stream), "device": ctx.device_name(), "rounds": args.rounds, "frames_per_s": {}}
for kw in MODES.values():
    one_pass(kw)                                       # warm-up: allocations, clocks
rates = {k: [] for k in MODES}
for r in range(args.rounds):                           # the modes alternate inside every round
    for k, kw in MODES.items():
        rates[k].append(one_pass(kw))
for k, v in rates.items():
    result["frames_per_s"][k] = {"per_round": [round(x[0], 1) for x in v], "median": round(float(np.median([x[0] for x in v])), 1),
                                 "accepted": [x[1] for x in v], "placed_by_the_map_step": [x[2] for x in v], "largest_map": max(x[3] for x in v)}
result["fused_over_unfused_per_round"] = [round(a[0] / b[0], 3) for a, b in zip(rates["map_fused"], rates["map"])]
result["fused_over_pair_per_round"] = [round(a[0] / b[0], 3) for a, b in zip(rates["map_fused"], rates["pair"])]
ctx.close()
if not args.no_kernels:
    hooks = os.path.abspath(os.path.join(HERE, "..", "openvo_amd", "libvo355_hooks.so"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-child", "--steps", str(args.steps)], env=dict(os.environ, VO355_LIB=hooks),
                         capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("KERNELS ")]
    if out.returncode != 0 or not lines:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        sys.exit(1)
    result["map_step_alone_us"] = json.loads(lines[-1][len("KERNELS "):])
print(json.dumps(result))
