"""Planted inputs of the patch alignment tests (tests/test_direct_kp_ref.py on the CPU, tests/test_gpu_direct_kp.py on the device).

The scenes are those of tests/direct_cases.py -- its textured plane, its rigs (the plain one and camera_cases.direct_rig), its PLANTED
pose and its renderer, imported, not copied.  What is new is the depth: instead of a disparity image a case carries KEYPOINTS, seeded
random float32 positions in pixels of the ROI crop, each with the 3-D point of the plane's ANALYTIC disparity at its (real) position
through Q, rounded to float32 -- what vo_sparse_stereo leaves in a slot.  Only the Z of a point is read by the alignment.

Every case carries its inputs, its keywords for direct_align_kp and the regime its name promises (`expect`); tests/test_direct_kp_ref.py
asserts, without a GPU, that the restatement (tests/direct_kp_ref.py) reaches that regime with a decision margin >= MARGIN (which here
also covers the distance of vx / 2^l, vy / 2^l from a rounding tie), which is what lets the device's integer fields be compared exactly.

Special keypoints (`special`), appended to or written over the random ones:
    dup        keypoint 1 is keypoint 0 again, keypoint 3 another position that rounds to keypoint 2's pixel at every level: both
               contribute, nothing is de-duplicated
    edge       four keypoints hp + 0.6 .. hp + 2.4 px from an edge of the crop: the patch fits level 0 alone; four 3 hp + 1.7 .. 3 hp + 3.4 px
               from one: it fits levels 0 and 1, not level 2; and five less than hp + 1 px from an edge, usable and in use at NO level.  The reverse -- a patch that fits a coarse level
               and not level 0 -- does not exist: the border a level asks for, (hp + 1) 2^l level-0 pixels, grows with l.
    bad        keypoints with a NaN, +inf, -inf, zero or negative Z and with a NaN, infinite, negative or beyond-the-image x or y among
               the good ones: skipped, never read (their positions would index far outside the image)

Seeds.  A case's seed (texture and keypoints) is changed until its margin holds, and the rejected seeds are written down here.
Rejected (margin below 1e-6 in the restatement): none -- the first seed tried for every case (its index in CASES + 41) held; the
margins are printed by tests/test_direct_kp_ref.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as CC                  # noqa: E402
import direct_cases as DC                  # noqa: E402

MARGIN = DC.MARGIN
PLANTED = DC.PLANTED


def plane_points(Q, xy_full, w, h, d0, ramp):
    """(n, 3) float64: the plane's points at full-image positions, through Q as the header reads it"""
    x, y = xy_full[:, 0].astype(np.float64), xy_full[:, 1].astype(np.float64)
    d = d0 + ramp[0] * (x - (w - 1) / 2.0) + ramp[1] * (y - (h - 1) / 2.0)
    W = Q[3, 2] * d + Q[3, 3]
    return np.stack([(x + Q[0, 3]) / W, (y + Q[1, 3]) / W, Q[2, 3] / W], 1)


class Case:
    def __init__(self, name, w, h, seed, n, kw, expect, roi=None, planted=True, special=(), **opt):
        self.name, self.w, self.h, self.seed, self.n, self.kw, self.expect, self.roi, self.planted = name, w, h, seed, n, dict(kw), expect, roi, planted
        self.special, self.opt = tuple(special), opt
        self._built = None

    def build(self):
        """-> (A, B, xy, xyz, Q, K4, Rt0, truth): built once, the arrays read-only.  xy (n, 2) float32 in pixels of the ROI crop,
        xyz (n, 3) float32"""
        if self._built is None:
            w, h, o = self.w, self.h, self.opt
            base = DC.Case(self.name, w, h, self.seed, {}, {}, **{k: v for k, v in o.items() if k in ("rig", "image", "occluder", "Rt0", "d0", "ramp")})
            A, B, _, Q, K4, Rt0, truth = base.build()
            d0, ramp = o.get("d0", 12.0), o.get("ramp", (0.03, 0.02))
            ox, oy = (0, 0) if self.roi is None else self.roi[:2]
            cw, ch = (w, h) if self.roi is None else (min(self.roi[2], w) - ox, min(self.roi[3], h) - oy)
            rng = np.random.default_rng([7, self.seed])
            xy = np.stack([rng.uniform(0, cw, self.n), rng.uniform(0, ch, self.n)], 1).astype(np.float32)
            hp = self.kw.get("patch", 5) // 2
            if "dup" in self.special:
                xy[1] = xy[0]
                xy[2] = np.float32([cw * 0.5 + 0.125, ch * 0.5 - 0.25])         # (both round to one pixel at every level up to 3)
                xy[3] = xy[2] + np.float32([0.0625, -0.03125])
            if "edge" in self.special:
                e = 0.137                                  # (keeps the fractions of cw and ch off the rounding ties)
                near = [(2.6 + hp - 2, ch * 0.3 + e), (cw - 4.4 - hp + 2, ch * 0.6 + e), (cw * 0.4 + e, 2.7 + hp - 2), (cw * 0.7 + e, ch - 4.3 - hp + 2),
                        (3 * hp + 1.7, ch * 0.45 + e), (cw - 3 * hp - 3.4, ch * 0.55 + e), (cw * 0.35 + e, 3 * hp + 1.7), (cw * 0.65 + e, ch - 3 * hp - 3.4)]
                out = [(0.3, ch * 0.5 + e), (cw - 0.6, ch * 0.4 + e), (cw * 0.5 + e, 0.2), (cw * 0.45 + e, ch - 0.7), (hp + 0.4, hp + 0.3)]
                xy = np.vstack([xy, np.float32(near), np.float32(out)])
            full = xy + np.float32([ox, oy])               # (float32, as the alignment adds the origin)
            with np.errstate(all="ignore"):
                xyz = plane_points(Q, full, w, h, d0, ramp).astype(np.float32)
            if "bad" in self.special:
                k = len(xy) // 2
                for i, z in enumerate((np.nan, np.inf, -np.inf, 0.0, -1.5)):
                    xyz[k + i, 2] = z
                for i, p in enumerate(((np.nan, 20.3), (20.3, np.nan), (np.inf, 10.3), (10.3, -np.inf), (-13.2, 20.3), (20.3, -9.7),
                                       (w + 40.2, 20.3), (20.3, h + 1000.2), (3.0e9, 3.0e9), (-3.0e9, 5.3))):
                    xy[k + 5 + i] = p
            for a in (xy, xyz):
                a.setflags(write=False)
            self._built = (A, B, xy, xyz, Q, K4, Rt0, truth)
        return self._built


_K = dict(levels=3, iters=8, patch=5, grad_min=4, huber=10.0, z_min=0.1, min_pixels=24)


def _k(**kw):
    return dict(_K, **kw)


_FAR = DC.pose((0.0, 0.0, 0.0), (1.4, 0.0, 0.0))        # (1.2, direct_cases' start, does not starve 200 patches: rejected)

# expect: status, and for status 0 "improves" (the planted cases), for the others the bounds on iters_done
CASES = [
    Case("p5_levels3", 96, 72, 41, 120, _k(), dict(status=0, improves=True)),
    Case("p3_levels4", 96, 72, 42, 300, _k(levels=4, patch=3, min_pixels=12), dict(status=0, improves=True)),
    Case("p7_levels2", 96, 72, 43, 60, _k(levels=2, patch=7), dict(status=0, improves=True)),
    Case("p5_levels1", 64, 48, 44, 40, _k(levels=1, iters=12), dict(status=0, improves=True)),
    Case("p3_levels2", 64, 48, 45, 150, _k(levels=2, patch=3), dict(status=0, improves=True)),
    Case("odd_p5_levels3", 97, 61, 46, 150, _k(), dict(status=0, improves=True)),
    Case("odd_p7_levels3", 97, 61, 47, 80, _k(patch=7, min_pixels=12), dict(status=0, improves=True)),
    Case("roi_p5", 96, 72, 48, 150, _k(), dict(status=0, improves=True), roi=(9, 6, 90, 67)),
    Case("huber_p5", 96, 72, 49, 200, _k(), dict(status=0, improves=True, huber=True), occluder=True),
    Case("tiny_p5", 96, 72, 50, 20, _k(levels=2, min_pixels=12), dict(status=0, improves=True, below_block=True)),
    Case("tiny_p3", 64, 48, 51, 40, _k(levels=2, patch=3, min_pixels=12), dict(status=0, improves=True, below_block=True)),
    Case("dup_p5", 96, 72, 52, 100, _k(), dict(status=0, improves=True), special=("dup",)),
    Case("edge_p5", 96, 72, 53, 100, _k(), dict(status=0, improves=True), special=("edge",)),
    Case("edge_p3_odd", 97, 61, 54, 100, _k(patch=3), dict(status=0, improves=True), special=("edge",)),
    Case("bad_p5", 96, 72, 55, 140, _k(), dict(status=0, improves=True), special=("bad",)),
    Case("bad_roi_p3", 96, 72, 56, 200, _k(patch=3), dict(status=0, improves=True), roi=(9, 6, 90, 67), special=("bad", "edge")),
    Case("none", 64, 48, 57, 0, _k(levels=2), dict(status=2, done=(0, 0)), planted=False),
    Case("constant", 96, 72, 58, 100, _k(), dict(status=2, done=(0, 0)), image="constant", planted=False),
    Case("starved_midway", 96, 72, 59, 200, _k(), dict(status=2, done=(1, 23)), planted=False, Rt0=_FAR),
    Case("bad_pivot", 96, 72, 60, 100, _k(levels=2), dict(status=-1, done=(0, 0)), image="columns", planted=False),
    # the generic rig (fx != fy, K4's principal point != Q's, Q[3][3] != 0)
    Case("generic_p5_levels3", 96, 72, 41, 120, _k(), dict(status=0, improves=True), rig="generic"),
    Case("generic_odd_p3", 97, 61, 46, 200, _k(patch=3), dict(status=0, improves=True), rig="generic"),
    Case("generic_small_p7", 64, 48, 45, 40, _k(levels=2, patch=7), dict(status=0, improves=True), rig="generic"),
    Case("generic_roi_p5", 96, 72, 48, 150, _k(), dict(status=0, improves=True), roi=(9, 6, 90, 67), rig="generic"),
]
BY_NAME = {c.name: c for c in CASES}
