"""Sparse stereo depth restated in numpy: the contract the sparse-stereo tests hold the kernels against (include/vo355.h,
vo_sparse_stereo, steps b - e), and the CPU odometer chain built on it.

    scales()                                   sc[o] = (float)pow((double)1.2f, o), o = 0 .. 7
    associate(...)                             step b: per left keypoint the accepted right keypoint or -1
    refine(...)                                step c: per left keypoint the refined disparity or NaN
    reproject(...)                             step d: cv2.reprojectImageTo3D's arithmetic on the float keypoint position
    sparse_stereo(...)                         b - e on two crops and their ORB keypoint dicts -> the compacted frame
    SparseRefOdometer                          the oracle odometer's state machine on such frames (both pose methods)

Every float32 / float64 operation is written out in the order the kernel evaluates it; the SADs are exact integers."""
import math

import numpy as np

W, L = 5, 5                 # half width of the SAD window, shifts -L .. L
KP_FIELDS = ("xy", "size", "angle", "response", "octave", "desc")


def scales():
    return np.array([np.float32(math.pow(float(np.float32(1.2)), o)) for o in range(8)], np.float32)


def hamming(a, b):
    """Hamming distances of one 32-byte descriptor against n of them"""
    return np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8)[None, :], np.asarray(b, np.uint8).reshape(-1, 32)), axis=1).sum(1).astype(np.int64)


def associate(xy_l, oct_l, desc_l, xy_r, oct_r, desc_r, min_disp, max_disp, row_tol, max_hamming):
    xy_l, xy_r = np.asarray(xy_l, np.float32).reshape(-1, 2), np.asarray(xy_r, np.float32).reshape(-1, 2)
    oct_l, oct_r = np.asarray(oct_l, np.int64).reshape(-1), np.asarray(oct_r, np.int64).reshape(-1)
    desc_l, desc_r = np.asarray(desc_l, np.uint8).reshape(-1, 32), np.asarray(desc_r, np.uint8).reshape(-1, 32)
    lo, hi, tolr, sc = np.float32(min_disp), np.float32(max_disp), np.float32(row_tol), scales()
    match = np.full(len(xy_l), -1, np.int32)
    if len(xy_r) == 0:
        return match
    for i in range(len(xy_l)):
        with np.errstate(invalid="ignore", over="ignore"):
            tol = tolr * sc[oct_l[i]]
            d0 = xy_l[i, 0] - xy_r[:, 0]
            assert tol.dtype == np.float32 and d0.dtype == np.float32
            cand = (np.abs(oct_l[i] - oct_r) <= 1) & (np.abs(xy_l[i, 1] - xy_r[:, 1]) <= tol) & (d0 >= lo) & (d0 <= hi)
        js = np.nonzero(cand)[0]
        if len(js) == 0:
            continue
        d = hamming(desc_l[i], desc_r[js])
        k = int(np.argmin(d * 65536 + js))                 # the lexicographically smallest (distance, j)
        if d[k] <= max_hamming:
            match[i] = js[k]
    return match


def refine_one(left, right, xl, yl, xr_f, min_disp, max_disp):
    """one accepted association -> float32 disparity or NaN; left / right: the two crops (same shape)"""
    nan = np.float32(np.nan)
    ch, cw = left.shape
    x0, y0, xr = int(np.rint(np.float32(xl))), int(np.rint(np.float32(yl))), int(np.rint(np.float32(xr_f)))     # half to even
    if x0 - W < 0 or x0 + W > cw - 1 or y0 - W < 0 or y0 + W > ch - 1:
        return nan
    if xr - (W + L) < 0 or xr + (W + L) > cw - 1:
        return nan
    patch = left[y0 - W:y0 + W + 1, x0 - W:x0 + W + 1].astype(np.int64)
    sad = [int(np.abs(patch - right[y0 - W:y0 + W + 1, xr + s - W:xr + s + W + 1].astype(np.int64)).sum()) for s in range(-L, L + 1)]
    k = int(np.argmin(sad))                                # the first minimum
    if k == 0 or k == 2 * L:
        return nan
    den = sad[k - 1] + sad[k + 1] - 2 * sad[k]
    if den <= 0:
        return nan
    delta = np.float32(sad[k - 1] - sad[k + 1]) / np.float32(2 * den)
    d = np.float32(x0 - xr - (k - L)) - delta
    assert d.dtype == np.float32
    if d > 0 and d >= np.float32(min_disp) and d <= np.float32(max_disp):
        return d
    return nan


def refine(left, right, xy_l, xy_r, match, min_disp, max_disp):
    xy_l, xy_r = np.asarray(xy_l, np.float32).reshape(-1, 2), np.asarray(xy_r, np.float32).reshape(-1, 2)
    disp = np.full(len(xy_l), np.nan, np.float32)
    for i, j in enumerate(match):
        if j >= 0:
            disp[i] = refine_one(left, right, xy_l[i, 0], xy_l[i, 1], xy_r[j, 0], min_disp, max_disp)
    return disp


def reproject(Q, xy, x0, y0, d):
    """xy (n, 2) float32 crop positions, d (n,) float32 -> (n, 3) float32"""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    xy, d = np.asarray(xy, np.float32).reshape(-1, 2), np.asarray(d, np.float32).reshape(-1)
    gx, gy = xy[:, 0] + np.float32(x0), xy[:, 1] + np.float32(y0)
    assert gx.dtype == np.float32
    v = [gx.astype(np.float64), gy.astype(np.float64), d.astype(np.float64), np.ones(len(d))]
    hg = []
    for r in range(4):
        s = np.zeros(len(d))
        for k in range(4):
            s = s + Q[r, k] * v[k]
        hg.append(s)
    with np.errstate(all="ignore"):
        ia = 1.0 / hg[3]
        return np.stack([(hg[r].astype(np.float32).astype(np.float64) * ia).astype(np.float32) for r in range(3)], 1)


def sparse_stereo(left, right, kl, kr, Q, x0, y0, min_disp, max_disp, row_tol=2.0, max_hamming=75):
    """left / right: the two crops; kl / kr: ORB keypoint dicts (xy, size, angle, response, octave, desc) in canonical order
    -> dict: the compacted left keypoints (same keys) + xyz, disp, keep (indices into kl), match, counts3"""
    if len(kr["xy"]) > 65535:
        raise ValueError("more than 65535 right keypoints")
    match = associate(kl["xy"], kl["octave"], kl["desc"], kr["xy"], kr["octave"], kr["desc"], min_disp, max_disp, row_tol, max_hamming)
    disp = refine(left, right, kl["xy"], kr["xy"], match, min_disp, max_disp)
    keep = np.nonzero(~np.isnan(disp))[0]
    out = {k: np.asarray(kl[k])[keep].copy() for k in KP_FIELDS}
    out["disp"] = disp[keep]
    out["xyz"] = reproject(Q, out["xy"], x0, y0, out["disp"])
    out.update(keep=keep, match=match, counts3=np.array([len(kl["xy"]), int((match >= 0).sum()), len(keep)], np.int32))
    return out


def crop_bounds(roi, w, h):
    """the rectangle vo_orb_detect_and_compute crops to: rows roi[1]:roi[3], columns roi[0]:roi[2] (numpy slice semantics)"""
    y0, y1, _ = slice(roi[1], roi[3]).indices(h)
    x0, x1, _ = slice(roi[0], roi[2]).indices(w)
    return x0, y0, max(x1, x0), max(y1, y0)


def sparse_frame(O, L, R, Q, roi, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75, orb=None):
    """one rectified pair through the oracle's ORB (or `orb(img) -> dict`) on both crops and the restatement"""
    h, w = L.shape
    x0, y0, x1, y1 = crop_bounds(roi, w, h)
    Lc, Rc = np.ascontiguousarray(L[y0:y1, x0:x1]), np.ascontiguousarray(R[y0:y1, x0:x1])
    orb = orb or (lambda img: O.orb_detect_and_compute(img, None, nfeatures))
    return sparse_stereo(Lc, Rc, orb(Lc), orb(Rc), Q, x0, y0, min_disp, max_disp, row_tol, max_hamming)


class SparseRefOdometer:
    """The reference odometer's state machine (oracle/odometer.py) with the sparse frames above as its depth source: the CPU chain
    the sparse odometer tests compare with.  pose_method "pnp": oracle ransac_pnp on (xyz of a, pixel of b); "umeyama": the oracle
    odometer's point_cloud_transform on (xyz of a, xyz of b).  cross_check / match_window as StereoOdometer defines them."""
    MIN_VALID_DISPARITY, MAX_VALID_DISPARITY = 4, 100

    def __init__(self, O, Q, roi, nfeatures=500, match_threshold=0.8, rigidity_threshold=0, outlier_threshold=0, min_matches=10,
                 pose_method="umeyama", pnp_iters=256, pnp_threshold=1.5, pnp_seed=4321, cross_check=False, match_window=None,
                 row_tol=2.0, max_hamming=75, frames=None):
        from oracle.odometer import RefStereoOdometer
        self.O, self.Q, self.roi, self.nfeatures = O, np.asarray(Q, np.float64), tuple(roi), nfeatures
        self.match_threshold, self.min_matches = match_threshold, min_matches
        self.pose_method, self.pnp = pose_method, (pnp_iters, pnp_threshold, pnp_seed)
        self.cross_check, self.match_window = cross_check, match_window
        self.row_tol, self.max_hamming = row_tol, max_hamming
        self._ref = RefStereoOdometer(None, nfeatures, match_threshold, rigidity_threshold, outlier_threshold, True, min_matches)
        self.frames = frames                    # optional cache: id of the left image -> sparse frame
        self.cur = self.prev = None
        self.skipped_frames = 0
        self.c_T_w, self.c_T_w_prev = np.eye(4), np.eye(4)
        self.skip_cause = ""
        self.log = []

    def frame(self, L, R):
        key = id(L)
        if self.frames is not None and key in self.frames:
            return self.frames[key]
        f = sparse_frame(self.O, L, R, self.Q, self.roi, self.nfeatures, self.MIN_VALID_DISPARITY, self.MAX_VALID_DISPARITY,
                         self.row_tol, self.max_hamming)
        x0, y0, _, _ = crop_bounds(self.roi, L.shape[1], L.shape[0])
        f["origin"] = (x0, y0)
        if self.frames is not None:
            self.frames[key] = f
        return f

    def matches(self, a, b, span):
        from window_match_ref import ratio_filter, window_knn2, window_knn2_mutual
        if self.match_window is None and not self.cross_check:
            idx, dist = self.O.bf_knn2_hamming(a["desc"], b["desc"])
            return self.O.ratio_filter(idx, dist, self.match_threshold)
        rx, ry = (np.inf, np.inf) if self.match_window is None else tuple(np.float32(r * span) for r in np.broadcast_to(self.match_window, 2))
        if self.cross_check:
            idx, dist, mutual, _ = window_knn2_mutual(a["desc"], b["desc"], a["xy"], b["xy"], rx, ry)
        else:
            idx, dist = window_knn2(a["desc"], b["desc"], a["xy"], b["xy"], rx, ry)
            mutual = np.ones(len(idx), np.uint8)
        q, t = ratio_filter(idx, dist, self.match_threshold)
        ok = mutual[q] > 0
        return q[ok], t[ok]

    def _gate(self, T):
        r = self._ref
        if np.isnan(T).any():
            self.skip_cause = "nan"
            return None
        lim = self.skipped_frames + 1
        big_d = np.linalg.norm(T[0:3, 3]) > r.MAX_DISTANCE_CHANGE * lim
        big_r = np.linalg.norm(self.O.rodrigues(T[0:3, 0:3])) > r.MAX_ROTATION_CHANGE * lim
        if big_d:
            self.skip_cause = "bigdist"
        if big_r:
            self.skip_cause = "bigrot"
        return None if big_d or big_r else T

    def try_pair(self, a, b, span):
        q, t = self.matches(a, b, span)
        self.log.append((len(a["xy"]), len(b["xy"]), len(q)))
        if len(q) < self.min_matches:
            self.skip_cause = "matches"
            return None
        if self.pose_method == "umeyama":
            r = self._ref
            r.skipped_frames, r.skip_cause = self.skipped_frames, self.skip_cause
            T = r.point_cloud_transform(a["xyz"][q], b["xyz"][t])
            self.skip_cause = r.skip_cause
            return T
        X = a["xyz"][q]
        ok = np.isfinite(X).all(axis=1)
        uv = b["xy"][t] + np.array(b["origin"], np.float32)
        if ok.sum() < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        Q = self.Q
        r = self.O.ransac_pnp(X[ok], uv[ok], [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]], *self.pnp)
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None
        return self._gate(np.vstack([r["Rt"], [0, 0, 0, 1]]))

    def update(self, L, R):
        nxt = self.frame(L, R)
        if len(nxt["xy"]) < self.min_matches:
            self.skipped_frames += 1
            self.skip_cause = "keypoints"
            return False
        if self.cur is None:
            self.cur = nxt
            return True
        T = self.try_pair(self.cur, nxt, self.skipped_frames + 1)
        if T is not None:
            self.c_T_w_prev = self.c_T_w
            self.c_T_w = T @ self.c_T_w
        elif self.prev is not None:
            T = self.try_pair(self.prev, nxt, self.skipped_frames + 2)
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

    def current_pose(self):
        return np.linalg.inv(self.c_T_w)
