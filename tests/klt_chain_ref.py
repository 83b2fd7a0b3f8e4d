"""CPU chains of StereoOdometer(match="klt"): the restatement's tracks (tests/klt_ref.py) in front of the oracle's RANSAC PnP /
Umeyama, inside the reference odometer's state machine.
  KltSparseRefOdometer   on the sparse frames of tests/sparse_stereo_ref.py (oracle ORB on both images): the chain the figures of
                         DESIGN 4k come from
  KltDenseChain          on per-frame data taken from the device (rectified left image, keypoints, disparity): the chain
                         tests/test_gpu_klt.py holds the odometer to"""
import numpy as np

import klt_ref as K
import sparse_stereo_ref as S


class KltSparseRefOdometer(S.SparseRefOdometer):
    def __init__(self, *a, klt=None, tracks=None, **kw):
        super().__init__(*a, pose_method="pnp", **kw)
        self.klt = dict(klt or {})
        self.tracks = tracks if tracks is not None else {}      # (id of a, id of b) -> tracks: shared between RANSAC seeds
        self.kept = []

    def frame(self, L, R):
        f = super().frame(L, R)
        f.setdefault("left", L)
        return f

    def try_pair(self, a, b, span):
        key = (id(a), id(b))
        if key not in self.tracks:
            self.tracks[key] = K.track(a["left"], b["left"], a["xy"], origin=a["origin"], **self.klt)
        xy, st, _ = self.tracks[key]
        idx = np.nonzero(st == 0)[0]
        self.kept.append((len(st), len(idx)))
        if len(idx) < self.min_matches:
            self.skip_cause = "matches"
            return None
        X = a["xyz"][idx]
        ok = np.isfinite(X).all(axis=1)
        uv = xy[idx] + np.array(b["origin"], np.float32)
        if ok.sum() < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        Q = self.Q
        r = self.O.ransac_pnp(np.ascontiguousarray(X[ok]), np.ascontiguousarray(uv[ok]), [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]], *self.pnp)
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None
        return self._gate(np.vstack([r["Rt"], [0, 0, 0, 1]]))


class KltDenseChain:
    """frames: dicts of left (the whole rectified image), xy (keypoints, crop pixels), disp16 (whole image, int16), in stream order.
    The state machine and the gates are the reference odometer's (oracle/odometer.py)."""

    def __init__(self, O, Q, roi, pose_method, klt, min_matches=10, pnp=(256, 1.5, 4321)):
        from oracle.odometer import RefStereoOdometer
        self.O, self.Q, self.roi, self.pose_method, self.klt, self.min_matches, self.pnp = O, np.asarray(Q, np.float64), tuple(roi), pose_method, klt, min_matches, pnp
        self._ref = RefStereoOdometer(None, 500, 0.8, 0, 0, True, min_matches)
        self.cur = self.prev = None
        self.skipped_frames = 0
        self.c_T_w, self.c_T_w_prev = np.eye(4), np.eye(4)
        self.skip_cause = ""
        self.counts = None
        self.tracks = {}

    _gate = S.SparseRefOdometer._gate

    def _lookup(self, f, xy):
        if not len(xy):
            return np.zeros((0, 3), np.float32), np.zeros(0, np.uint8)
        return self.O.points3d_at(f["disp16"], self.Q, self.roi, np.ascontiguousarray(xy, np.float32))

    def try_pair(self, a, b):
        x0, y0, x1, y1 = S.crop_bounds(self.roi, a["left"].shape[1], a["left"].shape[0])
        key = (id(a), id(b))
        if key not in self.tracks:
            self.tracks[key] = K.track(a["left"], b["left"], a["xy"], origin=(x0, y0), **self.klt)
        xy, st, _ = self.tracks[key]
        idx = np.nonzero(st == 0)[0]
        self.counts = (len(st), len(idx))
        if len(idx) < self.min_matches:
            self.skip_cause = "matches"
            return None
        pa, sa = self._lookup(a, a["xy"][idx])
        ok = (sa == 0) & np.isfinite(pa).all(axis=1)
        idx, pa = idx[ok], pa[ok]
        uv = xy[idx]
        if self.pose_method == "pnp":
            if len(idx) < max(self.min_matches, 4):
                self.skip_cause = "matches"
                return None
            Q = self.Q
            r = self.O.ransac_pnp(np.ascontiguousarray(pa), np.ascontiguousarray(uv + np.array([x0, y0], np.float32)),
                                  [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]], *self.pnp)
            if r["best_count"] < self.min_matches:
                self.skip_cause = "outlier"
                return None
            return self._gate(np.vstack([np.asarray(r["Rt"], np.float64).reshape(3, 4), [0, 0, 0, 1]]))
        inside = (uv[:, 0] >= 0) & (uv[:, 1] >= 0) & (uv[:, 0] < np.float32(x1 - x0)) & (uv[:, 1] < np.float32(y1 - y0))
        pa, uv = pa[inside], uv[inside]
        pb, sb = self._lookup(b, uv)
        ok = (sb == 0) & np.isfinite(pb).all(axis=1)
        pa, pb = pa[ok], pb[ok]
        if len(pa) < self.min_matches:
            self.skip_cause = "matches"
            return None
        r = self._ref
        r.skipped_frames, r.skip_cause = self.skipped_frames, self.skip_cause
        T = r.point_cloud_transform(pa, pb)
        self.skip_cause = r.skip_cause
        return T

    def update(self, nxt):
        if len(nxt["xy"]) < self.min_matches:
            self.skipped_frames += 1
            self.skip_cause = "keypoints"
            return False
        if self.cur is None:
            self.cur = nxt
            return True
        T = self.try_pair(self.cur, nxt)
        if T is not None:
            self.c_T_w_prev = self.c_T_w
            self.c_T_w = T @ self.c_T_w
        elif self.prev is not None:
            T = self.try_pair(self.prev, nxt)
            if T is not None:
                base = self.c_T_w_prev
                self.c_T_w_prev = self.c_T_w
                self.c_T_w = T @ base
                self.skipped_frames = 0
        if T is None:
            self.skipped_frames += 1
            return False
        self.skipped_frames = 0
        self.prev, self.cur = self.cur, nxt
        return True
