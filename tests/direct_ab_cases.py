"""Planted inputs of the tests of the dense direct alignment with the affine brightness term (tests/test_direct_ab_ref.py on the CPU,
tests/test_gpu_direct_ab.py on the device): the cases of tests/direct_cases.py at their shapes (96 x 72, 97 x 61, 64 x 48), with image B
sent through a grey-level TABLE before it is handed over -- the device the census work used to move the exposure of one image.

    identity   B untouched: the extra unknowns must cost nothing
    gain       rint(0.7 B + 40): the inverse is k = 1 / 0.7 = 1.4286, m = -40 / 0.7 = -57.14
    clip       clip(rint(1.25 B - 20), 0, 255): saturates at both ends (B < 16 and B > 220), the inverse is k = 0.8, m = 16 elsewhere
    inverted   255 - B: the best gain is negative, which the definition refuses (status -1 through k <= 0)

Cases: every planted case of direct_cases.CASES under the first three tables; `constant`, `starved_midway` and `bad_pivot` (B
untouched: `constant` and `bad_pivot` stop in the held iteration it = 0 of the coarsest level, `starved_midway` starves in its first
FREE iteration); iters = 3 variants, which have exactly ONE free iteration per level; `inverted`; and `held_starve`, whose gradient
threshold (14) leaves level 1 257 points and level 0 only 22 of the 24 it needs (the finer the level, the smaller the texture's
central difference), so that the step starves in a HELD iteration -- it = 0 of level 0 -- after six free iterations have moved
(k, m).  A constant B is deliberately NOT a case: its last pivot (the offset column against the gain column) is zero up to rounding,
so the decision would sit on its bound.

Every case carries `expect`: the status, for status 0 "improves", otherwise `stop` = (level, it) of the iteration that ended the
step and `done` = the iterations completed.  tests/test_direct_ab_ref.py asserts them with a decision margin >= MARGIN.

Seeds.  A case's seed is that of the case of direct_cases.py it is built from, to be changed until its margin holds, the rejected
seeds written down here.  Rejected (margin below 1e-6 in the restatement): none; tests/test_direct_ab_ref.py prints every margin."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_cases as DC                  # noqa: E402

MARGIN = DC.MARGIN
TABLES = {
    "identity": lambda B: B,
    "gain": lambda B: np.rint(0.7 * B.astype(np.float64) + 40.0).astype(np.uint8),
    "clip": lambda B: np.clip(np.rint(1.25 * B.astype(np.float64) - 20.0), 0, 255).astype(np.uint8),
    "inverted": lambda B: (255 - B.astype(np.int64)).astype(np.uint8),
}
INVERSE = {"identity": (1.0, 0.0), "gain": (1.0 / 0.7, -40.0 / 0.7), "clip": (0.8, 16.0)}      # (k, m) with k table(B) + m = B


class Case:
    def __init__(self, name, base, table, expect, seed=None, **kw):
        b = DC.BY_NAME[base]
        self.name, self.base, self.table, self.expect = name, base, table, dict(expect)
        self.w, self.h, self.roi, self.planted = b.w, b.h, b.roi, b.planted
        self.kw = dict(b.kw, **kw)
        self._src = b if seed is None else DC.Case(b.name, b.w, b.h, seed, b.kw, b.expect, roi=b.roi, planted=b.planted, **b.opt)
        self._built = None

    def build(self):
        """-> (A, B through the table, disp16, Q, K4, Rt0, truth): built once, the arrays read-only"""
        if self._built is None:
            A, B, disp, Q, K4, Rt0, truth = self._src.build()
            B = np.ascontiguousarray(TABLES[self.table](B))
            B.setflags(write=False)
            self._built = (A, B, disp, Q, K4, Rt0, truth)
        return self._built


_OK = dict(status=0, improves=True)
PLANTED = [c.name for c in DC.CASES if c.planted]
CASES = [Case("%s_%s" % (n, t), n, t, _OK) for t in ("identity", "gain", "clip") for n in PLANTED]
CASES += [
    Case("constant", "constant", "identity", dict(status=2, stop=(2, 0), done=0)),
    Case("starved_midway", "starved_midway", "identity", dict(status=2, stop=(2, 2), done=2)),       # starves in the first FREE iteration
    Case("bad_pivot", "bad_pivot", "identity", dict(status=-1, stop=(1, 0), done=0)),
    # exactly one free iteration per level
    Case("levels3_gain_iters3", "levels3", "gain", dict(status=0), iters=3),
    Case("small_clip_iters3", "small", "clip", dict(status=0), iters=3),
    Case("generic_odd_levels3_gain_iters3", "generic_odd_levels3", "gain", dict(status=0), iters=3),
    Case("levels1_identity_iters3", "levels1", "identity", dict(status=0), iters=3),
    # k <= 0 at the first free iteration: nothing of that iteration is committed
    Case("inverted", "levels3", "inverted", dict(status=-1, stop=(2, 2), done=2)),
    # starves in a held iteration, after free ones
    Case("held_starve", "levels2", "gain", dict(status=2, stop=(0, 0), done=8), grad_min=14),
]
BY_NAME = {c.name: c for c in CASES}
