"""The references of the planted-dense-slot tests (tests/planted_dense.py) on the CPU: the numpy restatement of the depth lookup
against the CPU oracle bit for bit, the regimes the inputs are named after (computed, never assumed from the construction) and the
restatement against the same definition in np.longdouble.  (That only the test-only library exports the planting entry is
asserted in tests/test_planted_ref.py, beside the sparse seam.)

Figures this file prints (see the docstring of tests/planted_dense.py): the largest deviation of the restatement from the
longdouble evaluation in float32 ulps, asserted below planted_dense.ULP_BOUND."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planted_dense as D                  # noqa: E402


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build_oracle()
    return O


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _roi4(roi):
    return (0, 0, 1 << 20, 1 << 20) if roi is None else roi       # (the oracle clips the far edge by the image, as the slice does)


def _same_lookup(got, st, want, wst, what):
    """status exact; bits equal wherever status != 2 (a NaN is a NaN: its sign is the platform's)"""
    assert np.array_equal(st, wst), "%s: status differs" % (what,)
    k = wst != 2
    nan = np.isnan(want[k])
    assert np.array_equal(np.isnan(got[k]), nan), "%s: NaN masks differ" % (what,)
    assert np.array_equal(_bits(got[k])[~nan], _bits(want[k])[~nan]), "%s: %d values differ in their bits" % (what, int((_bits(got[k])[~nan] != _bits(want[k])[~nan]).sum()))
    assert np.isnan(got[~k]).all()


@pytest.mark.parametrize("field,qname,roiname", D.COMBOS, ids=["-".join(c) for c in D.COMBOS])
def test_restatement_equals_the_oracle(oracle, field, qname, roiname):
    disp, Q, roi = D.FIELDS[field](), D.QS[qname], D.ROIS[roiname]
    for s in D.POSITIONS:
        xy = D.positions(s, disp, Q, roi)
        got, st = D.lookup(disp, Q, roi, xy)
        want, wst = oracle.points3d_at(disp, Q, _roi4(roi), xy)
        _same_lookup(got, st, want, wst, (field, qname, roiname, s))
    for n in (1, 63, 64, 65, 300):
        xy = D.mixed_positions(disp, Q, roi, n)
        assert len(xy) == n
        _same_lookup(*D.lookup(disp, Q, roi, xy), *oracle.points3d_at(disp, Q, _roi4(roi), xy), (field, qname, roiname, n))


@pytest.mark.parametrize("size", [(D.W, D.H), (67, 33), (300, 21)])
def test_per_pixel_part_equals_the_oracle(oracle, size):
    """the sizes of the download tests: row tails of the 256-wide blocks, two blocks per row"""
    for field in D.FIELDS:
        disp = D.FIELDS[field](*size)
        for qname, Q in D.QS.items():
            got, want = D.reproject(disp, Q), oracle.reproject_to_3d(disp.astype(np.float32) / np.float32(16.0), Q)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (field, qname, size)
            assert np.isinf(want).any() == (D.HOLE16[qname] in disp), (field, qname)


def _classes():
    for field, qname, roiname in D.COMBOS:
        disp, Q, roi = D.FIELDS[field](), D.QS[qname], D.ROIS[roiname]
        for s in D.POSITIONS:
            xy = D.positions(s, disp, Q, roi)
            yield field, qname, roiname, s, D.classify(disp, Q, roi, xy)


def test_every_named_regime_is_hit_by_the_set_named_after_it():
    hit = {}
    for field, qname, roiname, s, c in _classes():
        def mark(name, mask):
            if np.any(mask):
                hit.setdefault(name, set()).add((field, qname, roiname, s))
        for k in range(5):
            mark("holes%d" % k, (c["holes"] == k) & (c["exist"] == 4))
        for k in (0, 1, 2):
            mark("status%d" % k, c["status"] == k)
        for k, e in enumerate(D.EDGE_NAMES):
            mark(e, c["edge"] == k)
            mark(e + "_hole", (c["edge"] == k) & (c["holes"] > 0))
        mark("renormalised", (c["status"] == 0) & (c["holes"] > 0))
        mark("invalid_tap", c["invalid"] & (c["status"] == 0))
        mark("mixed_signs", c["mixed"])
        mark("w_zero_at_nonzero_disparity", c["wzero"])
        mark("clipped_edge", c["clipped"] and (c["edge"] > 0).any())
        mark("origin_edge", roiname == "inner" and (c["edge"] > 0).any())
    def of(name, s, field=None, q=None, roi=None):
        return [h for h in hit.get(name, ()) if h[3] == s and all(v is None or h[i] == v for i, v in enumerate((field, q, roi)))]
    for roiname in D.ROIS:              # every ROI meets every hole count, both bad statuses and every edge kind
        for k in range(5):
            assert of("holes%d" % k, "hole_counts", field="hole_blocks", q="plain", roi=roiname), (k, roiname)
            assert of("holes%d" % k, "hole_counts", field="w_zero", q="w33", roi=roiname), (k, roiname)
        assert of("status1", "on_hole", field="single_holes", roi=roiname) and of("status2", "on_hole", field="hole_band", roi=roiname)
        assert of("status2", "integer", field="hole_band", roi=roiname) and of("status2", "float", field="hole_band", roi=roiname)
        for e in D.EDGE_NAMES[1:]:
            assert of(e, "edges", roi=roiname), (e, roiname)
        assert of("last_column_hole", "edges", roi=roiname) or of("last_row_hole", "edges", roi=roiname), roiname     # an edge AND a skipped tap
        for s in ("half", "quarter", "float"):
            assert of("renormalised", s, field="hole_blocks", roi=roiname), (s, roiname)
    assert of("clipped_edge", "edges", roi="clipped") and of("origin_edge", "edges", roi="inner")
    assert of("invalid_tap", "float", field="invalid") and of("mixed_signs", "float", field="invalid", q="plain")
    assert of("w_zero_at_nonzero_disparity", "on_hole", field="w_zero", q="w33") and of("status1", "on_hole", field="w_zero", q="w33")
    assert not hit.get("w_zero_at_nonzero_disparity", set()) - {h for h in hit["w_zero_at_nonzero_disparity"] if h[1] == "w33"}
    # under the Q[3,3] != 0 matrix a ZERO disparity is no hole: the field of zero holes has none there
    assert not of("status2", "on_hole", field="hole_band", q="w33") and not of("holes1", "hole_counts", field="single_holes", q="w33")
    print("regimes hit: " + ", ".join("%s (%d)" % (k, len(v)) for k, v in sorted(hit.items())))


def test_restatement_against_longdouble():
    worst, where, n_used = 0.0, None, 0
    for field, qname, roiname in D.COMBOS:
        disp, Q, roi = D.FIELDS[field](), D.QS[qname], D.ROIS[roiname]
        for s in D.POSITIONS:
            xy = D.positions(s, disp, Q, roi)
            if not len(xy):
                continue
            got, st = D.lookup(disp, Q, roi, xy)
            c = D.classify(disp, Q, roi, xy)
            k = (st == 0) & ~c["mixed"]
            ex = D.exact(disp, Q, roi, xy)[k]
            ulp = np.spacing(np.abs(ex).astype(np.float32)).astype(np.longdouble)
            d = float((np.abs(got[k].astype(np.longdouble) - ex) / ulp).max()) if k.any() else 0.0
            n_used += int(k.sum())
            if d > worst:
                worst, where = d, (field, qname, roiname, s)
    print("restatement - longdouble: at most %.3g float32 ulps over %d keypoints (at %s)" % (worst, n_used, where))
    assert n_used > 10000 and worst <= D.ULP_BOUND


def test_pose_cases_reach_their_regimes(oracle):
    seen = set()
    for c in D.POSE_CASES:
        c.build()
        for disp, xy, xyz, st in ((c.disp_a, c.xy_a, c.xyz_a, c.st_a), (c.disp_b, c.xy_b, c.xyz_b, c.st_b)):
            _same_lookup(xyz, st, *oracle.points3d_at(disp, c.Q, _roi4(c.roi), xy), c.name)     # (the twin's points ARE the oracle's)
        m = c.model(oracle)
        M, n1, n2, flags = m["counts"]
        sa, sb = c.st_a[m["q"]], c.st_b[m["t"]]
        cl = D.classify(c.disp_a, c.Q, c.roi, c.xy_a[m["q"]])
        fl = c.dense_flags(m)
        print("%s: (M, n1, n2, flags) = (%d, %d, %d, %d) rc %s; status 1 / 2 among the matches: %d / %d; renormalised %d" % (
            c.name, M, n1, n2, fl, m["rc"], int((sa == 1).sum() + (sb == 1).sum()), int((sa == 2).sum() + (sb == 2).sum()),
            int(((cl["status"] == 0) & (cl["holes"] > 0)).sum())))
        assert M == c.M
        eb = D.classify(c.disp_b, c.Q, c.roi, c.xy_b[m["t"]])
        if c.edge:
            assert ((eb["edge"] == 1) & (eb["status"] == 0)).sum() >= 10 and n1 >= 10 and m["rc"][1] == 0, c.name     # partners in the last column, and a fit
        assert m["cond"] > 1e-6, c.name
        if c.holes == "none" and not c.edge:
            assert not sa.any() and not sb.any() and fl == 0 and n1 == M and n2 >= 10 and m["rc"] == (0, 0), c.name
            assert np.abs(m["T2"][:, :3] - np.eye(3)).max() < 1e-6 and abs(m["T2"][0, 3] - D.SHIFT[0] / (D.QS[c.qname][3, 2] * D.PLANES16[c.qname][0] / 16.0 + D.QS[c.qname][3, 3])) < 1e-6
        if c.holes == "renorm":
            assert ((cl["status"] == 0) & (cl["holes"] > 0)).sum() >= 10 and n1 >= 10 and m["rc"][1] == 0, c.name
        if c.holes in ("status1", "both"):
            assert (sa == 1).any() and (sb == 1).any(), c.name
            assert (fl & 2) == (2 if c.rigidity == 0 else 0), c.name
        if c.holes in ("status2", "both"):
            assert (sa == 2).any() and fl & 1, c.name
        else:
            assert not fl & 1, c.name
        if c.rigidity > 0:
            assert n1 >= 10 and m["rc"][1] == 0, c.name         # the clique filter removes the NaN points: a fit is reached
        seen.add((c.qname, c.roiname, c.holes, c.rigidity > 0))
        if c.edge:
            seen.add(("edge", c.roiname))
    assert {("edge", r) for r in D.ROIS} <= seen
    seen = {s for s in seen if len(s) == 4}
    assert {s[0] for s in seen} == set(D.QS) and {s[1] for s in seen} == set(D.ROIS) and {s[2] for s in seen} == {"none", "renorm", "status1", "status2", "both"}
    assert any(c.nq > 256 for c in D.POSE_CASES)                # more than one stride of the 256-thread lookup loop


def test_pnp_cases_reach_their_regimes(oracle):
    reg = set()
    for c in D.PNP_CASES:
        c.build()
        _same_lookup(c.xyz_a, c.st_a, *oracle.points3d_at(c.disp_a, c.Q, _roi4(c.roi), c.xy_a), c.name)
        m = c.model(oracle)
        st = c.st_a[m["mq"]]
        use = st == 0
        assert np.array_equal(use, m["ok"]), c.name               # the finite filter IS the status filter: status != 0 <=> a NaN coordinate
        cl = D.classify(c.disp_a, c.Q, c.roi, c.xy_a[m["q"]])    # the usable ones: renormalised taps and the last column among them
        assert (cl["status"] == 0).all() and (m["n"] < 40 or ((cl["holes"] > 0).sum() >= 5 and (cl["edge"] == 1).sum() >= 3)), c.name
        flags = int((st == 2).any())
        print("%s: (M, n, flags) = (%d, %d, %d), status 1 / 2 among the matches %d / %d, best %d @ %d" % (
            c.name, m["M"], m["n"], flags, int((st == 1).sum()), int((st == 2).sum()), m["best_count"], m["best_iter"]))
        if not c.cross:
            assert m["M"] == c.M and m["n"] == c.n, c.name
            assert np.array_equal(np.flatnonzero(~use), c.bad), c.name
        else:
            assert m["M"] < c.M and m["n"] < m["M"], c.name       # the cross-check removed the duplicates
        if len(c.bad):
            assert (st == 1).any() and (st == 2).any() and flags == 1, c.name
        else:
            assert flags == 0
        if m["n"] >= 4:
            assert m["best_count"] >= 0.5 * m["n"], c.name        # the planted motion is found
        else:
            assert m["best_count"] == 0
        for w in range(0, m["M"], 64):
            if not use[w:w + 64].any() and len(use[w:w + 64]) == 64:
                reg.add("wave_unusable")
        reg.add("M<=256" if m["M"] <= 256 else "M>=257")
        if m["M"] >= 257 and not use[:256].any():
            reg.add("pass0_unusable")
        if m["n"] < 4:
            reg.add("n<4")
        reg.add("flag0_%d" % flags)
        if c.roi is not None:
            assert not np.array_equal(m["uv"], c.xy_b[m["t"]]) and np.array_equal(m["uv"], c.xy_b[m["t"]] + np.float32([3, 5]))
            if (m["uv"].astype(np.float64) != c.xy_b[m["t"]].astype(np.float64) + [3.0, 5.0]).any():
                reg.add("uv_add_rounds")                          # the float32 add is not exact for some partner
    print("regimes: %s" % sorted(reg))
    assert reg >= {"M<=256", "M>=257", "wave_unusable", "pass0_unusable", "n<4", "flag0_0", "flag0_1", "uv_add_rounds"}
