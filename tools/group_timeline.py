"""Diagnostic: do other pairs' fronts run while a sweep group's chain runs?  (DESIGN 4f'')

C2 through StereoOdometer.update() in the environment as it is (GPU_MAX_HW_QUEUES is NOT touched: with few hardware queues the
look-ahead pairs travel in sweep groups), 12 warm-up pairs, then 60 pairs with every stage timed.  The stage timers record a
HIP event pair per stage on the stage's own stream (vo_get_stage_timeline), so -- unlike a kernel trace, which serialises the
dispatches -- they show what overlaps.  Per group: the chain interval (begin of the group's W + E bracket to the end of its
post-filter bracket) and how many cost-volume / ORB brackets of OTHER pairs begin inside it (a batched front bracket counts as
its members), with the microseconds of them that lie inside.  Last line: the share of chain time during which at least one such bracket was running.
The events cost throughput: never part of a rate.   Usage: python tools/group_timeline.py [steady pairs, default 60]"""
import gc
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openvo_amd import StereoCamera, StereoOdometer
from openvo_amd.synth import Corridor
import bench

K, W = int(sys.argv[1]) if len(sys.argv) > 1 else 60, 12
c = Corridor("C2")
cam = StereoCamera(c.K(), c.dist(), c.K(), c.dist(), c.rect_params(), c.sgbm_params(), (c.w, c.h), max_keypoints=500)
odo = StereoOdometer(cam, **bench.ODO_KW)
staged = cam.stage_pairs(c.pairs(0, W + K))
ctx = cam._ctx
gc.collect()
gc.disable()
for i in range(W):
    odo.update(staged[i], None)
ctx.enable_timing(True)
for i in range(W, W + K):
    odo.update(staged[i], None)
ctx.synchronize()
tl = ctx.stage_timeline()
ctx.enable_timing(False)
print("GPU_MAX_HW_QUEUES=%s engines %d sweep group %d lib %s: %d brackets over %.2f ms" % (
    os.environ.get("GPU_MAX_HW_QUEUES", "unset"), ctx.set_engines(), ctx.set_sweep_group(), os.environ.get("VO355_LIB", "(this tree)"),
    len(tl), max(e for (_, _, _, e) in tl) - min(b for (_, _, b, _) in tl) if tl else 0.0))

# a group's launches are recorded back to back when it closes: W + E, sweep, post filters (and its ORB chain where the
# group carries it), each bracket with entries = members
chains, own = [], set()
for i, (st, n, b, e) in enumerate(tl):
    if st == "sgbm_agg" and n > 1 and i + 2 < len(tl) and tl[i + 1][0] == "sgbm_wta" and tl[i + 2][0] == "sgbm_post" and tl[i + 1][1] == n and tl[i + 2][1] == n:
        own.update((i, i + 1, i + 2))
        orb = None
        if i + 3 < len(tl) and tl[i + 3][0] == "orb" and tl[i + 3][1] == n:
            own.add(i + 3)
            orb = tl[i + 3]
        chains.append((n, b, tl[i + 2][3], orb))
# (a bracket of another group's batched fronts -- one planes launch and one cost launch for n members, VO_GROUP_FRONTS -- counts
# as n fronts)
fronts = [(st, n, b, e) for i, (st, n, b, e) in enumerate(tl) if i not in own and st in ("sgbm_cost", "orb")]
tot_chain = tot_cover = 0.0
for g, (n, b, e, orb) in enumerate(chains):
    inside = {"sgbm_cost": [0, 0.0], "orb": [0, 0.0]}
    cover = []
    for (st, fn, fb, fe) in fronts:
        lo, hi = max(fb, b), min(fe, e)
        if b <= fb < e:
            inside[st][0] += max(fn, 1)
        if hi > lo:
            inside[st][1] += (hi - lo) * 1e3
            cover.append((lo, hi))
    cover.sort()
    covered, at = 0.0, b
    for (lo, hi) in cover:
        if hi > at:
            covered += hi - max(lo, at)
            at = hi
    tot_chain += e - b
    tot_cover += covered
    print("group %2d: %2d members, chain %8.3f .. %8.3f ms (%6.0f us)%s | other pairs' sgbm_cost: %2d begin inside, %6.0f us inside | orb: %2d begin inside, %6.0f us inside | covered %3.0f %%" % (
        g, n, b, e, (e - b) * 1e3, (", own ORB chain to %8.3f" % orb[3]) if orb else "", inside["sgbm_cost"][0], inside["sgbm_cost"][1],
        inside["orb"][0], inside["orb"][1], 100.0 * covered / (e - b) if e > b else 0.0))
print("summary: %d groups, chain time %.2f ms, of which another pair's front (sgbm_cost / orb) was running during %.2f ms = %.1f %%" % (
    len(chains), tot_chain, tot_cover, 100.0 * tot_cover / tot_chain if tot_chain > 0 else 0.0))
