"""The association tests of the sparse stereo chain and the temporal loop check restated in numpy (include/vo355.h:
vo_set_sparse_assoc, vo_set_match_loop), on top of tests/sparse_stereo_ref.py, which stays as it is.

    associate_ex(..., flags, ratio)            step b with the ratio and the mutual test -> (match, a) -- a[j]: the claim word of right keypoint j
    sparse_stereo_ex(..., flags, ratio)        b - e with them -> the compacted frame plus rdesc (the right partner's descriptor)
    loop_gate(a, b, q, t, max_hamming)         the loop check on matches (q, t) of two such frames
    SparseLoopOdometer                         SparseRefOdometer with the association tests in frame() and the loop gate in matches()

flags: bit 0 = mutual, bit 1 = ratio (VO_SPARSE_MUTUAL / VO_SPARSE_RATIO)."""
import numpy as np

import sparse_stereo_ref as S

MUTUAL, RATIO = 1, 2
NO_CLAIM = 0xFFFFFFFF


def associate_ex(xy_l, oct_l, desc_l, xy_r, oct_r, desc_r, min_disp, max_disp, row_tol, max_hamming, flags=0, ratio=None):
    """-> (match (nl,) int32, a (nr,) uint32).  a[j] = the smallest (distance << 16 | i) over the left keypoints i that have j as a
    candidate at a distance <= max_hamming (NO_CLAIM: none), computed whatever the flags; match is step b's winner where it
    passes the threshold and every enabled test, -1 elsewhere."""
    xy_l, xy_r = np.asarray(xy_l, np.float32).reshape(-1, 2), np.asarray(xy_r, np.float32).reshape(-1, 2)
    oct_l, oct_r = np.asarray(oct_l, np.int64).reshape(-1), np.asarray(oct_r, np.int64).reshape(-1)
    desc_l, desc_r = np.asarray(desc_l, np.uint8).reshape(-1, 32), np.asarray(desc_r, np.uint8).reshape(-1, 32)
    lo, hi, tolr, sc = np.float32(min_disp), np.float32(max_disp), np.float32(row_tol), S.scales()
    nl, nr = len(xy_l), len(xy_r)
    if (flags & MUTUAL) and nl > 65535:
        raise ValueError("more than 65535 left keypoints with the mutual test")
    match = np.full(nl, -1, np.int32)
    a = np.full(nr, NO_CLAIM, np.uint32)
    if nr == 0:
        return match, a
    if flags & RATIO:
        r32 = np.float32(ratio)
        assert np.float32(0) < r32 <= np.float32(1)
    for i in range(nl):
        with np.errstate(invalid="ignore", over="ignore"):
            tol = tolr * sc[oct_l[i]]
            d0 = xy_l[i, 0] - xy_r[:, 0]
            cand = (np.abs(oct_l[i] - oct_r) <= 1) & (np.abs(xy_l[i, 1] - xy_r[:, 1]) <= tol) & (d0 >= lo) & (d0 <= hi)
        js = np.nonzero(cand)[0]
        if len(js) == 0:
            continue
        d = S.hamming(desc_l[i], desc_r[js])
        near = d <= max_hamming
        if i <= 65535:
            a[js[near]] = np.minimum(a[js[near]], (d[near] * 65536 + i).astype(np.uint32))
        order = np.argsort(d * 65536 + js)                  # lexicographic (distance, j)
        d1, j1 = int(d[order[0]]), int(js[order[0]])
        ok = d1 <= max_hamming
        if ok and (flags & RATIO) and len(js) > 1:
            d2 = int(d[order[1]])                           # the runner-up, whatever its distance
            prod = r32 * np.float32(d2)
            assert prod.dtype == np.float32
            ok = bool(np.float32(d1) < prod)
        if ok:
            match[i] = j1
    if flags & MUTUAL:
        for i in np.nonzero(match >= 0)[0]:
            if (int(a[match[i]]) & 0xFFFF) != i:
                match[i] = -1
    return match, a


def sparse_stereo_ex(left, right, kl, kr, Q, x0, y0, min_disp, max_disp, row_tol=2.0, max_hamming=75, flags=0, ratio=None):
    """S.sparse_stereo with the association tests; the result carries rdesc = kr["desc"][match[keep]] as well, and disp_all (nl,):
    the refined disparity of every left keypoint, NaN where it has none"""
    if len(kr["xy"]) > 65535:
        raise ValueError("more than 65535 right keypoints")
    match, _ = associate_ex(kl["xy"], kl["octave"], kl["desc"], kr["xy"], kr["octave"], kr["desc"], min_disp, max_disp, row_tol, max_hamming,
                            flags, ratio)
    disp = S.refine(left, right, kl["xy"], kr["xy"], match, min_disp, max_disp)
    keep = np.nonzero(~np.isnan(disp))[0]
    out = {k: np.asarray(kl[k])[keep].copy() for k in S.KP_FIELDS}
    out["disp"] = disp[keep]
    out["xyz"] = S.reproject(Q, out["xy"], x0, y0, out["disp"])
    out["rdesc"] = np.asarray(kr["desc"], np.uint8).reshape(-1, 32)[match[keep]].copy()
    out.update(keep=keep, match=match, disp_all=disp, counts3=np.array([len(kl["xy"]), int((match >= 0).sum()), len(keep)], np.int32))
    return out


def sparse_frame_ex(O, L, R, Q, roi, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75, flags=0, ratio=None, orb=None):
    """S.sparse_frame through sparse_stereo_ex"""
    h, w = L.shape
    x0, y0, x1, y1 = S.crop_bounds(roi, w, h)
    Lc, Rc = np.ascontiguousarray(L[y0:y1, x0:x1]), np.ascontiguousarray(R[y0:y1, x0:x1])
    orb = orb or (lambda img: O.orb_detect_and_compute(img, None, nfeatures))
    return sparse_stereo_ex(Lc, Rc, orb(Lc), orb(Rc), Q, x0, y0, min_disp, max_disp, row_tol, max_hamming, flags, ratio)


def loop_gate(a, b, q, t, max_hamming):
    """matches (q, t) between frames a and b -> those whose right partners are within max_hamming of each other"""
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    if len(q) == 0:
        return q, t
    d = np.unpackbits(np.bitwise_xor(a["rdesc"][q], b["rdesc"][t]), axis=1).sum(1)
    ok = d <= max_hamming
    return q[ok], t[ok]


class SparseLoopOdometer(S.SparseRefOdometer):
    """SparseRefOdometer whose frames come from sparse_stereo_ex (mutual / ratio) and whose matches pass the loop gate (loop_check:
    None or the threshold 0 .. 256; it is not scaled with the frames a pair spans)"""

    def __init__(self, *args, mutual=False, ratio=None, loop_check=None, **kw):
        super().__init__(*args, **kw)
        self.flags = (MUTUAL if mutual else 0) | (RATIO if ratio is not None else 0)
        self.ratio, self.loop_check = ratio, loop_check

    def frame(self, L, R):
        key = id(L)
        if self.frames is not None and key in self.frames:
            return self.frames[key]
        f = sparse_frame_ex(self.O, L, R, self.Q, self.roi, self.nfeatures, self.MIN_VALID_DISPARITY, self.MAX_VALID_DISPARITY,
                            self.row_tol, self.max_hamming, self.flags, self.ratio)
        x0, y0, _, _ = S.crop_bounds(self.roi, L.shape[1], L.shape[0])
        f["origin"] = (x0, y0)
        if self.frames is not None:
            self.frames[key] = f
        return f

    def matches(self, a, b, span):
        q, t = super().matches(a, b, span)
        if self.loop_check is None:
            return q, t
        return loop_gate(a, b, q, t, self.loop_check)
