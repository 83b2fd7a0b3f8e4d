"""The fused map step (include/vo355.h, vo_track_map) restated in numpy on top of tests/map_ref.py, which it imports and leaves alone:

    padded_view(map, ...)                      step a: MapRef.view's rows, then rows [vis, n) as clones of row 0 with a NaN point
    decide(...)                                step c: the decision codes in their order
    compose(T, P) / rigid_inverse(cw)          step d: the bracketed 4x4 product and the rigid inverse, as explicit sums (no `@`)
    update_dev(map, ...)                       step d: MapRef.update fed from the step's own arrays, with the kernel's range checks
    track(map, frame, ...)                     the whole step around a PnP function
    MapFusedRefOdometer                        MapRefOdometer whose map step is track()

Every float64 operation is written in the order the kernels evaluate it; nothing here shares code with them."""
import math

import numpy as np

import map_ref as M

TRACK_MAX = 3800
CAUSES = {0: "", 1: None, 2: "matches", 3: "matches", 4: "outlier", 5: "nan", 6: "bigdist", 7: "bigrot"}      # decision -> skip_cause
NAN32 = np.float32(np.nan)


def padded_view(m, Rt_cw, K4, z_min, origin, crop_wh):
    """-> MapRef.view's dict with n = len(map) rows in xy / xyz / desc / rdesc / octave (src and counts2 as there) + vis"""
    v = m.view(Rt_cw, K4, z_min, origin, crop_wh)
    n, vis = len(m), len(v["src"])
    pad = n - vis
    if vis:
        row = dict(xy=v["xy"][:1], desc=v["desc"][:1], rdesc=v["rdesc"][:1], octave=v["octave"][:1])
    else:
        row = dict(xy=np.zeros((1, 2), np.float32), desc=np.zeros((1, 32), np.uint8), rdesc=np.zeros((1, 32), np.uint8), octave=np.zeros(1, np.int32))
    out = dict(v, vis=vis)
    for k in ("xy", "desc", "rdesc", "octave"):
        out[k] = np.concatenate([v[k], np.repeat(row[k], pad, axis=0)]).astype(v[k].dtype)
    out["xyz"] = np.concatenate([v["xyz"], np.full((pad, 3), NAN32, np.float32)]).astype(np.float32)
    return out


def gate_figures(T):
    """-> (|t|, angle) of a 3x4 pose as the decision kernel computes them"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    t0, t1, t2 = float(T[0, 3]), float(T[1, 3]), float(T[2, 3])
    dist = math.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
    a, b, c = float(T[2, 1]) - float(T[1, 2]), float(T[0, 2]) - float(T[2, 0]), float(T[1, 0]) - float(T[0, 1])
    s = math.sqrt((a * a + b * b) + c * c) / 2.0
    co = (((float(T[0, 0]) + float(T[1, 1])) + float(T[2, 2])) - 1.0) / 2.0
    return dist, math.atan2(s, co)


def decide(vis, matches, flags, n, best_count, T, min_matches, max_dist, max_rot):
    """the decision code of the step (T: the 3x4 pose the gates see -- the refined one when the refinement succeeded)"""
    if vis < max(min_matches, 2) or vis > TRACK_MAX:
        return 1
    if matches < min_matches:
        return 2
    if flags & 2:
        return 8
    if n < max(min_matches, 4):
        return 3
    if best_count < min_matches:
        return 4
    T = np.asarray(T, np.float64).reshape(3, 4)
    if np.isnan(T).any():
        return 5
    with np.errstate(all="ignore"):
        dist, angle = gate_figures(T)
    dec = 0
    if dist > max_dist:
        dec = 6
    if angle > max_rot:
        dec = 7                        # (the last cause set wins, as in _gate)
    return dec


def compose(T, P):
    """T . P for two 3x4 poses read as 4x4 matrices with the last row (0, 0, 0, 1): four-term sums, left to right -> 3x4"""
    T, P = np.asarray(T, np.float64).reshape(3, 4), np.asarray(P, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            last = 1.0 if j == 3 else 0.0
            out[i, j] = ((float(T[i, 0]) * float(P[0, j]) + float(T[i, 1]) * float(P[1, j])) + float(T[i, 2]) * float(P[2, j])) + float(T[i, 3]) * last
    return out


def rigid_inverse(cw):
    """[R^T | -(R^T t)] of a 3x4 pose, the three-term sums left to right"""
    cw = np.asarray(cw, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = cw[j, i]
        out[i, 3] = -((float(cw[0, i]) * float(cw[0, 3]) + float(cw[1, i]) * float(cw[1, 3])) + float(cw[2, i]) * float(cw[2, 3]))
    return out


def update_dev(m, frame, wc, serial, max_age, max_obs, q, t, mask, vis, accept):
    """-> (counts6, update_flags).  Not accepted: six times -1 and the map untouched.  An inlier whose q is not below vis or whose t
    is not below the frame's keypoint count (as unsigned numbers): flag 1, six times -1, the map untouched."""
    none = np.full(6, -1, np.int32)
    if not accept:
        return none, 0
    q, t, mask = np.asarray(q, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1), np.asarray(mask).reshape(-1) != 0
    nk = len(np.asarray(frame["xyz"]).reshape(-1, 3))
    uq, ut = q[mask] & 0xFFFFFFFF, t[mask] & 0xFFFFFFFF
    if (uq >= vis).any() or (ut >= nk).any():
        return none, 1
    assert len(m.view_src) == vis
    return m.update(frame, wc, serial, max_age, max_obs, q[mask], t[mask], np.ones(int(mask.sum()), np.uint8)), 0


def track(m, frame, Rt_cw_pred, K4, z_min, origin, crop_wh, pnp, min_matches, max_dist, max_rot, serial, max_age, max_obs):
    """The step on MapRef m.  pnp(view, frame) -> dict(matches, flags, n, best_count, Rt, Rt_refined, refine_status, q, t, mask) for
    the PADDED view it is handed (it must look at the first view["vis"] rows only behind the matcher).  -> the record"""
    if len(m) > TRACK_MAX:
        raise ValueError("a map of more than %d landmarks" % TRACK_MAX)
    view = padded_view(m, Rt_cw_pred, K4, z_min, origin, crop_wh)
    vis = view["vis"]
    if len(m) == 0:
        return dict(decision=1, view=np.array([0, 0], np.int32), update=np.full(6, -1, np.int32), update_flags=0, c_T_w=np.zeros((3, 4)), w_T_c=np.zeros((3, 4)))
    r = pnp(view, frame)
    T = r["Rt_refined"] if r.get("refine_status", 1) == 0 else r["Rt"]
    dec = decide(vis, r["matches"], r["flags"], r["n"], r["best_count"], T, min_matches, max_dist, max_rot)
    cw, wc = np.zeros((3, 4)), np.zeros((3, 4))
    if dec == 0:
        cw = compose(T, Rt_cw_pred)
        wc = rigid_inverse(cw)
    counts, uflags = update_dev(m, frame, wc, serial, max_age, max_obs, r["q"], r["t"], r["mask"], vis, dec == 0)
    return dict(r, decision=dec, view=np.array([view["counts2"][0], vis], np.int32), update=counts, update_flags=uflags, c_T_w=cw, w_T_c=wc)


class MapFusedRefOdometer(M.MapRefOdometer):
    """MapRefOdometer whose map step is the fused one: the matcher sees the PADDED view, everything behind it the first vis rows;
    decisions by decide(), c_T_w by compose(), the map's pose by rigid_inverse().  The pairwise fallback and the fold without
    observations are MapRefOdometer's."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.decisions = []

    def _pnp(self, view, b):
        vis = view["vis"]
        q, t = self.matches(view, b, self.skipped_frames + 1)
        keep = q < vis                                   # the ratio test and everything behind it see the first vis rows only
        q, t = q[keep], t[keep]
        self.log.append((vis, len(b["xy"]), len(q)))
        out = dict(matches=len(q), flags=0, n=0, best_count=0, Rt=np.zeros((3, 4)), q=np.zeros(0, np.int64), t=np.zeros(0, np.int64),
                   mask=np.zeros(0, np.uint8))
        X = view["xyz"][q]
        ok = np.isfinite(X).all(axis=1)
        uv = b["xy"][t] + np.array(b["origin"], np.float32)
        out.update(n=int(ok.sum()), q=q[ok], t=t[ok], mask=np.zeros(int(ok.sum()), np.uint8))
        if ok.sum() >= 4:
            r = self.O.ransac_pnp(X[ok], uv[ok], self._K4(), *self.pnp)
            out.update(best_count=int(r["best_count"]), Rt=np.asarray(r["Rt"], np.float64).reshape(3, 4), mask=r["mask"])
        return out

    def update(self, L, R):
        nxt = self.frame(L, R)
        if len(nxt["xy"]) < self.min_matches:
            self.skipped_frames += 1
            self.skip_cause = "keypoints"
            return False
        if self.cur is None:
            self.map.reset()
            self.serial = 0
            self.cur = nxt
            self.track_source = None
            self._fold(nxt)
            return True
        h, w = L.shape
        from sparse_stereo_ref import crop_bounds
        x0, y0, x1, y1 = crop_bounds(self.roi, w, h)
        span = self.skipped_frames + 1
        ref = self._ref
        r = track(self.map, nxt, self.c_T_w[:3], self._K4(), self.z_min, (x0, y0), (x1 - x0, y1 - y0), self._pnp, self.min_matches,
                  ref.MAX_DISTANCE_CHANGE * span, ref.MAX_ROTATION_CHANGE * span, self.serial, self.max_age, self.max_obs)
        self.map_counts["view"] = r["view"]
        self.decisions.append(r["decision"])
        if r["decision"] == 0:
            self.c_T_w_prev = self.c_T_w
            self.c_T_w = np.vstack([r["c_T_w"], [0, 0, 0, 1]])
            self.skipped_frames = 0
            self.prev, self.cur = self.cur, nxt
            self.track_source = "map"
            self.map_counts["update"] = r["update"]
            self.serial += 1
            self.sizes.append(len(self.map))
            return True
        if CAUSES[r["decision"]] is not None:
            self.skip_cause = CAUSES[r["decision"]]
        ok = self._pairwise(nxt)
        if ok:
            self.track_source = "pair"
            self._fold(nxt)
        return ok
