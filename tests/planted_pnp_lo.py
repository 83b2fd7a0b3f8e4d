"""Inputs and the model for the planted-slot tests of the PnP step's local-optimisation rounds (vo_pnp_pair_lo: the LO form of
k_pnp_finish in csrc/ransac.hip).  No GPU in here; tests/planted_pnp.py supplies the cases' construction and the RANSAC model,
tests/pnp_lo_ref.py the restatement of the rounds.

A case is a planted_pnp.PnpCase whose pixel noise (about one pixel) puts correspondences on both sides of the 1.5 px threshold, so
that the set grows and shrinks from round to round, together with the (rounds, steps) pairs it is run with.  lo_model(case, O,
rounds, steps) runs the restatement three ways -- sequential sums, thread-strided sums (the order a thread of k_pnp_finish meets its
points in), np.longdouble sums -- and admitted() is the ADMISSION CONDITION of a case: all three give the same float32 P and the
same set in every round.  A flipped last bit of P moves the float32 test by about 1e-5 of the threshold; a case with a point that
near the edge is not a test of the kernel but of the summation order, and is replaced.  tests/test_pnp_lo_ref.py asserts the
condition for every case on the CPU; tests/test_gpu_planted_pnp_lo.py holds the kernel to the model.

Regimes, from the LO form of k_pnp_finish (one block of 256 threads):
    n usable 6 | 7                       the gate of a round (>= 6 points), a set that can fall below it
    n usable 255 | 256 | 257 | 603       one point per thread at most | a second trip of the strided re-selection loop, its ballot
                                         with lanes beyond n, the four waves' counts in LDS
    inliers at i >= 256 only             the first trip of the loop counts nothing
    support crossing 6                   a round completes and leaves fewer than 6 points: the next cannot run (c < R)
    rounds 1, 2, 3, 8 x steps 1, 3, 5    R = 1 is the plain refit; 8 the bound"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted_pnp as PP                   # noqa: E402
import pnp_lo_ref as PL                    # noqa: E402
from planted_pnp import PnpCase            # noqa: E402

GRID = [(r, s) for r in (1, 2, 3, 8) for s in (1, 3, 5)]
# The scene seeds of the three small cases were found by the loops of test_pnp_lo_ref.py::test_the_small_scenes_can_be_found_again:
# N6: all six of six in the winner's set; N7: the winner holds 6 of the 7 and the refit wins the seventh back; CROSS: the winner
# holds 6 of 12, the refit loses one of them -- round 1 completes with 5 points and round 2 cannot run.
N6_SCENE, N7_SCENE, CROSS_SCENE = 1, 22, 2
MARGIN = 1e-4          # the nearest point to the threshold, relative: ten times what one bit of P moves the test by (see above)


class RingCase(PnpCase):
    """PnpCase whose inliers sit ON a ring of `ring` pixels around their projection (direction drawn per scene) instead of in a
    Gaussian cloud: every inlier is near the threshold, so a refit that spreads the error can push one of them over it."""

    def __init__(self, *a, ring=1.35, **kw):
        super().__init__(*a, noise=0.0, **kw)
        self.ring = ring

    def build(self):
        if hasattr(self, "dq"):
            return self
        super().build()
        rng = np.random.default_rng([77, self.scene])
        inl = self.inl_pos
        phi = rng.uniform(0, 2 * np.pi, len(inl))
        uv = PP.project(self.xyz_a[self.q0[inl]]) + self.ring * np.stack([np.cos(phi), np.sin(phi)], 1)
        self.xy_b[self.t0[inl]] = uv.astype(np.float32)
        return self


def _cases():
    kw = dict(noise=1.0, refine=3)
    return [
        (PnpCase("n6_all_planted", 9, 6, n_in=6, noise=0.5, refine=3, scene=N6_SCENE), GRID),
        (PnpCase("n7_six_grow_to_seven", 10, 7, n_in=7, noise=0.8, refine=3, scene=N7_SCENE), GRID),
        (RingCase("support_crosses_6", 15, 12, n_in=8, refine=3, scene=CROSS_SCENE, ring=1.35), [(1, 3), (2, 3), (3, 1), (8, 5)]),
        (PnpCase("n255", 258, 255, n_in=180, **kw), [(1, 3), (2, 1), (3, 3), (8, 5)]),
        (PnpCase("n256", 259, 256, n_in=180, **kw), [(1, 5), (2, 3), (3, 1), (8, 3)]),
        (PnpCase("n257", 260, 257, n_in=180, **kw), [(1, 1), (2, 5), (3, 3), (8, 1)]),
        (PnpCase("n603", 606, 603, n_in=420, **kw), [(2, 5), (3, 3)]),
        (PnpCase("inliers300_second_pass_on", 603, 600, n_in=300, inliers=range(256, 556), **kw), [(2, 1), (3, 3)]),
    ]


CASES = _cases()
ALL = [(c.name, r, s) for c, runs in CASES for r, s in runs]


def case(name):
    return next(c for c, _ in CASES if c.name == name)


def lo_model(c, O, rounds, steps):
    """-> dict(Rt, mask, status, steps, rounds, support: the restatement with sequential sums; trace, trace_strided, trace_ld:
    (P, S_r) per completed round of the three runs; Rt_strided, Rt_ld; margin: the smallest relative distance of a point from the
    threshold over the rounds)"""
    key = (rounds, steps)
    cache = c.__dict__.setdefault("_lo", {})
    if key in cache:
        return cache[key]
    m = c.model(O)
    a = (m["Rt"], m["mask"], m["X"], m["uv"], c.K4, PP.THR, steps, rounds)
    t0, t1, t2 = [], [], []
    Rt, S, status, nsteps, done = PL.lo(*a, trace=t0)
    Rs, Ss, st_s, _, done_s = PL.lo(*a, order=PP.strided_order, trace=t1)
    Rl, Sl, st_l, _, done_l = PL.lo(*a, dtype=np.longdouble, trace=t2)
    margin = min([PL.select_margin(P, m["X"], m["uv"], PP.THR) for P, _ in t0] or [float("inf")])
    out = dict(Rt=Rt, mask=S, status=status, steps=nsteps, rounds=done, support=int(S.sum()), trace=t0, trace_strided=t1, trace_ld=t2,
               Rt_strided=Rs, Rt_ld=Rl, others=((st_s, done_s), (st_l, done_l)), margin=margin)
    cache[key] = out
    return out


def admitted(lm):
    """the admission condition: the three runs completed the same rounds with the same float32 P and the same set in each (and,
    stricter than asked: no point nearer to the threshold than MARGIN in any round)"""
    if not lm["margin"] >= MARGIN:
        return False
    if any(o != (lm["status"], lm["rounds"]) for o in lm["others"]):
        return False
    for other in (lm["trace_strided"], lm["trace_ld"]):
        if len(other) != len(lm["trace"]):
            return False
        for (P, S), (P2, S2) in zip(lm["trace"], other):
            if not (np.array_equal(P.view(np.uint32), P2.view(np.uint32)) and np.array_equal(S, S2)):
                return False
    return True
