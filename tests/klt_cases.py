"""Planted inputs of the Lucas-Kanade tests (tests/test_klt_ref.py on the restatement, tests/test_gpu_klt.py on the kernels): the two
textures, the point lists and the committed fixture tests/golden/klt_corridor_t0.npz."""
import os

import numpy as np

import klt_ref as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "klt_corridor_t0.npz")
# The smooth texture's seed.  The seed is part of the planted input, chosen on the CPU with the restatement: over seeds 1 .. 12 the worst
# of 200 points of the 96 x 64 / win 9 / 2 levels / (2.5, -1.25) case lies between 0.05 and 0.17 px (a 9 x 9 window sees half a period
# of the highest frequency, and the images are rounded to 8 bits); 6 is one of the textures that keep every case of
# test_klt_ref.py inside the issue's 0.1 px.
SMOOTH_SEED = 6
SHAPES = ((96, 64, 9, 2), (97, 65, 5, 3), (160, 120, 21, 3), (160, 120, 31, 1))      # (w, h, win, levels) of the GPU cases
WG_POINTS = 4                                                                       # points per workgroup of k_klt_track
COUNTS = (0, 1, WG_POINTS - 1, WG_POINTS, WG_POINTS + 1, 257)
OSC_PARAMS = dict(win=9, levels=2)                                                  # under which the fixture's osc_xy oscillate


def flat_rect(w, h):
    """x, y, width, height of the flat patch of the smooth pair: wider than the largest window of that shape plus its taps"""
    s = 40 if w >= 160 else 22
    return w // 4, h // 4, s, s


def corridor_crops():
    """the 160 x 120 crops of the left images of frames 0 and 1 of corridor T0 (rendered: needs the synthetic renderer)"""
    from openvo_amd.synth import Corridor
    (l0, _), (l1, _) = Corridor("T0").pairs(0, 2)
    return np.ascontiguousarray(l0[60:180, 80:240]), np.ascontiguousarray(l1[60:180, 80:240])


def find_oscillating(a, b, n=300, seed=3):
    """points of the crop pair whose forward track ends a level by the oscillation stop (and is tracked) under OSC_PARAMS"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(2, a.shape[1] - 3, n), rng.uniform(2, a.shape[0] - 3, n)], 1).astype(np.float32)
    tr = {}
    _, st, _ = K.track(a, b, xy, fb=0, trace=tr, **OSC_PARAMS)
    return xy[(tr["osc"] > 0) & (st == 0)]


def make_fixture(path=GOLDEN):
    a, b = corridor_crops()
    np.savez_compressed(path, a=a, b=b, osc_xy=find_oscillating(a, b)[:8])


def fixture():
    z = np.load(GOLDEN)
    return z["a"], z["b"], z["osc_xy"]


def smooth_pair(w, h, shift=(2.5, -1.25), flat=True):
    """the smooth texture and its shifted copy; with `flat`, a constant patch in both (a point on it has no gradient)"""
    a, b = K.smooth_texture(w, h, seed=SMOOTH_SEED), K.smooth_texture(w, h, shift, seed=SMOOTH_SEED)
    if flat:
        x, y, fw, fh = flat_rect(w, h)
        a[y:y + fh, x:x + fw] = 90
        b[y:y + fh, x:x + fw] = 90
    return a, b


def corridor_pair(w, h):
    a, b, _ = fixture()
    return np.ascontiguousarray(a[:h, :w]), np.ascontiguousarray(b[:h, :w])


def points(w, h, n, seed=11, extra=()):
    """n points, the special ones first: sub-pixel interior, a corner, NaN, the flat patch, inf, then every border and corner within
    2 px, points just outside the image and a far one, `extra`, and random sub-pixel points over the whole image"""
    F = flat_rect(w, h)
    fx, fy = F[0] + F[2] / 2.0, F[1] + F[3] / 2.0
    sp = [(w * 0.5 + 0.37, h * 0.5 - 0.21), (1.3, 0.7), (np.nan, 10.0), (fx + 0.25, fy - 0.5), (np.inf, 5.0),
          (w - 1.6, h - 2.0), (0.0, h - 1.0), (w - 1.0, 0.0), (w * 0.5, 1.9), (w * 0.5, h - 2.5), (0.4, h * 0.5), (w - 1.25, h * 0.5),
          (w - 1.0, h - 1.0), (0.0, 0.0), (-1.5, h * 0.5), (w + 0.75, h + 3.0), (12.0, -np.inf), (-3.0e6, 2.0e9), (3.0e38, -3.0e38),
          (fx, fy), (F[0] + 0.5, F[1] + 0.5)]
    sp += [tuple(p) for p in extra]
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-1, w, max(n, 1)), rng.uniform(-1, h, max(n, 1))], 1)
    return np.concatenate([np.array(sp, np.float64), rnd])[:n].astype(np.float32).reshape(-1, 2)


def same_bits(a, b):
    """bit-for-bit equality of two arrays of one dtype (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
