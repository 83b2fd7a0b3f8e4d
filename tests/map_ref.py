"""The landmark map restated in numpy: the contract the map tests hold the two kernels against (include/vo355.h, vo_map_view and
vo_map_update), and the CPU odometer chain that tracks against such a map.

    transform(Rt, p)                           T(Rt, p) of the header: float32 points through float64, the sums bracketed as there
    MapRef                                     the map: view(), update(), reset(), download(); ValueError where the library refuses
    MapRefOdometer                             SparseRefOdometer's frames and decisions with the map step as the first attempt

Every float32 / float64 operation is written out in the order the kernels evaluate it; nothing here shares code with them."""
import numpy as np

from sparse_stereo_ref import SparseRefOdometer

FIELDS = ("xyz", "desc", "rdesc", "octave", "obs", "last")


def transform(Rt, p):
    """Rt: 3x4 float64; p (n, 3) float32 -> (n, 3) float32"""
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(((Rt[i, 0] * x + Rt[i, 1] * y) + Rt[i, 2] * z) + Rt[i, 3]).astype(np.float32) for i in range(3)], 1)


def _empty(n=0):
    return dict(xyz=np.zeros((n, 3), np.float32), desc=np.zeros((n, 32), np.uint8), rdesc=np.zeros((n, 32), np.uint8),
                octave=np.zeros(n, np.int32), obs=np.zeros(n, np.int32), last=np.zeros(n, np.int32))


class MapRef:
    def __init__(self, capacity, kp_cap=None):
        kp_cap = capacity if kp_cap is None else kp_cap
        if not 16 <= capacity <= kp_cap:
            raise ValueError("need 16 <= capacity <= kp_cap")
        self.capacity, self.kp_cap = int(capacity), int(kp_cap)
        self.reset()

    def reset(self):
        self.m = _empty()
        self.view_src = np.zeros(0, np.int32)      # the last view: void after every update, reset and plant
        self.max_serial = -1

    def __len__(self):
        return len(self.m["xyz"])

    def plant(self, xyz, desc, rdesc, octave, obs, last):
        """n landmarks as they stand (any float32 bits as positions), as the test-only entry of the library plants them"""
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        if n > self.capacity:
            raise ValueError("more landmarks than capacity")
        self.m = dict(xyz=xyz.copy(), desc=np.asarray(desc, np.uint8).reshape(n, 32).copy(), rdesc=np.asarray(rdesc, np.uint8).reshape(n, 32).copy(),
                      octave=np.asarray(octave, np.int32).reshape(n).copy(), obs=np.asarray(obs, np.int32).reshape(n).copy(),
                      last=np.asarray(last, np.int32).reshape(n).copy())
        if n and (self.m["last"].min() < 0 or self.m["obs"].min() < 1):
            raise ValueError("need last >= 0 and obs >= 1")
        self.view_src = np.zeros(0, np.int32)
        self.max_serial = int(self.m["last"].max()) if n else -1

    def download(self):
        return {k: self.m[k].copy() for k in FIELDS}

    def view(self, Rt_cw, K4, z_min, origin, crop_wh):
        """-> dict(xy (k, 2), xyz (k, 3) camera coordinates, desc, rdesc, octave, src (the landmark of each keypoint), counts2)"""
        Rt_cw, K4 = np.asarray(Rt_cw, np.float64).reshape(-1)[:12].reshape(3, 4), np.asarray(K4, np.float64).reshape(4)
        z_min = np.float32(z_min)
        if not (np.isfinite(Rt_cw).all() and np.isfinite(K4).all() and K4[0] > 0 and K4[1] > 0 and np.isfinite(z_min) and z_min >= 0):
            raise ValueError("need a finite pose, finite K4 with positive focal lengths and a finite z_min >= 0")
        fx, fy, cx, cy = K4
        m = self.m
        Xc = transform(Rt_cw, m["xyz"])
        with np.errstate(all="ignore"):
            X0, X1, X2 = (Xc[:, k].astype(np.float64) for k in range(3))
            u = (fx * (X0 / X2) + cx).astype(np.float32) - np.float32(origin[0])
            v = (fy * (X1 / X2) + cy).astype(np.float32) - np.float32(origin[1])
            assert u.dtype == np.float32 and v.dtype == np.float32
            vis = (np.isfinite(Xc).all(axis=1) & (Xc[:, 2] >= z_min) & (u >= 0) & (u <= np.float32(crop_wh[0] - 1))
                   & (v >= 0) & (v <= np.float32(crop_wh[1] - 1)))
        src = np.nonzero(vis)[0].astype(np.int32)
        self.view_src = src
        return dict(xy=np.stack([u[src], v[src]], 1), xyz=Xc[src], desc=m["desc"][src].copy(), rdesc=m["rdesc"][src].copy(),
                    octave=m["octave"][src].copy(), src=src.copy(), counts2=np.array([len(self), len(src)], np.int32))

    def update(self, frame, Rt_wc, serial, max_age, max_obs, q=(), t=(), mask=()):
        """frame: dict(xyz (nk, 3) float32, desc, octave[, rdesc]) -- the keypoints of the tracked frame.  -> counts6"""
        Rt_wc = np.asarray(Rt_wc, np.float64).reshape(-1)[:12].reshape(3, 4)
        q, t, mask = np.asarray(q, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1), np.asarray(mask).reshape(-1) != 0
        f_xyz = np.asarray(frame["xyz"], np.float32).reshape(-1, 3)
        nk = len(f_xyz)
        f_desc, f_oct = np.asarray(frame["desc"], np.uint8).reshape(nk, 32), np.asarray(frame["octave"], np.int32).reshape(nk)
        f_rdesc = np.asarray(frame["rdesc"], np.uint8).reshape(nk, 32) if frame.get("rdesc") is not None else np.zeros((nk, 32), np.uint8)
        if not len(q) == len(t) == len(mask) or len(q) > self.kp_cap:
            raise ValueError("q, t and mask: one length, at most kp_cap")
        if max_age < 0 or not 1 <= max_obs <= 65535:
            raise ValueError("need max_age >= 0 and 1 <= max_obs <= 65535")
        if serial < 0 or serial < self.max_serial:
            raise ValueError("the serial is negative or below one used before")
        if not np.isfinite(Rt_wc).all():
            raise ValueError("the pose is not finite")
        if ((q < 0) | (q >= len(self.view_src))).any():
            raise ValueError("a q outside the last view")
        if ((t < 0) | (t >= nk)).any():
            raise ValueError("a t outside the frame")
        if len(np.unique(q[mask])) != int(mask.sum()):
            raise ValueError("a view keypoint named twice among the inliers")
        m = self.m
        Xo = transform(Rt_wc, f_xyz)
        fin = np.isfinite(Xo).all(axis=1)
        claimed = np.zeros(nk, bool)
        observed = skipped = 0
        # 1. observations
        for c in np.nonzero(mask)[0]:
            l, k = int(self.view_src[q[c]]), int(t[c])
            if not fin[k]:
                skipped += 1
                continue
            w = np.float64(min(int(m["obs"][l]), max_obs) + 1)
            old = m["xyz"][l].astype(np.float64)
            m["xyz"][l] = (old + (Xo[k].astype(np.float64) - old) / w).astype(np.float32)
            m["obs"][l] += 1
            m["last"][l] = serial
            m["desc"][l], m["rdesc"][l], m["octave"][l] = f_desc[k], f_rdesc[k], f_oct[k]
            claimed[k] = True
            observed += 1
        # 2. survivors
        keep = np.nonzero(serial - m["last"].astype(np.int64) <= max_age)[0]
        culled = len(self) - len(keep)
        # 3. insertions
        want = np.nonzero(~claimed & fin)[0]
        room = self.capacity - len(keep)
        ins = want[:room]
        new = dict(xyz=Xo[ins], desc=f_desc[ins], rdesc=f_rdesc[ins], octave=f_oct[ins], obs=np.ones(len(ins), np.int32),
                   last=np.full(len(ins), serial, np.int32))
        # 4. the other set
        self.m = {k: np.concatenate([m[k][keep], new[k]]).astype(m[k].dtype) for k in FIELDS}
        self.view_src = np.zeros(0, np.int32)
        self.max_serial = int(serial)
        return np.array([observed, skipped, culled, len(ins), len(want) - len(ins), len(self)], np.int32)


class MapRefOdometer(SparseRefOdometer):
    """SparseRefOdometer (pose_method "pnp") that tracks against a MapRef: the state machine of StereoOdometer(track="map").  Every
    decision, skip_cause and gate is the pairwise chain's; only the first attempt -- the PnP step on (view of the map under c_T_w,
    new frame) -- is new, and the map receives every accepted frame."""

    def __init__(self, O, Q, roi, max_age=5, max_obs=8, z_min=0.1, capacity=2000, **kw):
        kw.setdefault("pose_method", "pnp")
        if kw["pose_method"] != "pnp":
            raise ValueError("the map chain needs pose_method='pnp'")
        super().__init__(O, Q, roi, **kw)
        self.map = MapRef(capacity)
        self.max_age, self.max_obs, self.z_min = max_age, max_obs, z_min
        self.serial = 0
        self.track_source = None
        self.map_counts = {}
        self.sizes = []

    def _K4(self):
        Q = self.Q
        return [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]

    def _map_step(self, view, b):
        """the decisions of SparseRefOdometer.try_pair (pnp) on (view, b) -> (T or None, q, t, mask of the usable correspondences)"""
        q, t = self.matches(view, b, self.skipped_frames + 1)
        self.log.append((len(view["xy"]), len(b["xy"]), len(q)))
        if len(q) < self.min_matches:
            self.skip_cause = "matches"
            return None, None, None, None
        X = view["xyz"][q]
        ok = np.isfinite(X).all(axis=1)
        uv = b["xy"][t] + np.array(b["origin"], np.float32)
        if ok.sum() < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None, None, None, None
        r = self.O.ransac_pnp(X[ok], uv[ok], self._K4(), *self.pnp)
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None, None, None, None
        return self._gate(np.vstack([r["Rt"], [0, 0, 0, 1]])), q[ok], t[ok], r["mask"]

    def _fold(self, nxt, q=(), t=(), mask=()):
        self.map_counts["update"] = self.map.update(nxt, np.linalg.inv(self.c_T_w)[:3], self.serial, self.max_age, self.max_obs, q, t, mask)
        self.serial += 1
        self.sizes.append(len(self.map))

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
        view = self.map.view(self.c_T_w[:3], self._K4(), self.z_min, (x0, y0), (x1 - x0, y1 - y0))
        self.map_counts["view"] = view["counts2"]
        T = None
        if len(view["xy"]) >= max(self.min_matches, 2):
            T, q, t, mask = self._map_step(view, nxt)
        if T is not None:
            self.c_T_w_prev = self.c_T_w
            self.c_T_w = T @ self.c_T_w
            self.skipped_frames = 0
            self.prev, self.cur = self.cur, nxt
            self.track_source = "map"
            self._fold(nxt, q, t, mask)
            return True
        ok = self._pairwise(nxt)
        if ok:
            self.track_source = "pair"
            self._fold(nxt)
        return ok

    def _pairwise(self, nxt):
        """today's two attempts, unchanged (SparseRefOdometer.update behind the frame extraction)"""
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
