"""The Lucas-Kanade kernels (openvo_amd/csrc/klt.hip) held to the DEFINITION of tests/klt_def.py -- float64, whole images, real
interpolation, nothing shared with the kernels' tap-by-tap form or its restatement -- on the cases of tests/klt_def_cases.py:

    pyramid      every level of both images, read back through vo_test_klt_level of the test-only library, EQUAL to the definition on
                 widths and heights around the kernel's tile edges and below 3
    one step     levels = 1, iters = 1, eps = 0, min_eig = 0, fb = 0 from starts with three fractional bits: p0 + delta under the bound
                 derived in klt_def's docstring, every kernel instantiation, the corridor's upper levels as images, the plaid whose sums
                 pass 2^31 and 2^32
    narrow, extreme   images narrower than the window and 0 / 255 stripes: bit for bit with the restatement AND held by the definition
    eigenvalue, forward-backward   min_eig / fb on both sides of the definitional value
    whole tracks      within TAU (measured between definition and restatement on the CPU, never on the kernel) under the caps
    the export   its refusals

tests/test_klt_def.py holds the restatement to the same on the CPU and shows that each check can refuse (the mutants).  All device calls
are made by ONE child process on one small context with VO355_LIB pointing at the test-only library; it only calls and stores, every
comparison is made here, after the caps of the case were asserted on the definition alone."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_cases as C                      # noqa: E402
import klt_def as D                        # noqa: E402
import klt_def_cases as DC                 # noqa: E402
import klt_ref as K                        # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_ARG, VO_E_STATE, VO_E_CAP = -1, -3, -4
CTX_W, CTX_H = 160, 120
READ_BACK = ("track-corridor-win31-l4", "track-smooth-win21-l3")       # besides the pyramid cases: the levels of these calls are read back


def _levels_of(case):
    return case["prm"]["levels"] if case["kind"] == "pyr" or case["name"] in READ_BACK else 0


# ------------------------------------------------------------------------------------------------ in the child process
def _device_body(path):
    from openvo_amd import _native
    ctx = _native.Context(0, CTX_W, CTX_H, 32, 400)
    lib, p = ctx._lib, _native._p
    out = {}
    buf = np.full((16, 16), 0xEE, np.uint8)
    codes = {"fresh": lib.vo_test_klt_level(ctx._h, 0, 0, 16, 16, p(buf))}        # the workspace was never prepared
    for case in DC.cases():
        xy_out, st, it = ctx.klt_track_host(case["a"], case["b"], case["xy"], **case["prm"])
        out[case["name"] + "|xy"], out[case["name"] + "|st"], out[case["name"] + "|it"] = xy_out, st, it
        h, w = case["a"].shape
        for l, (wl, hl) in enumerate(DC.level_sizes(w, h, _levels_of(case))):
            for which in (0, 1):
                out["%s|L%d%d" % (case["name"], which, l)] = ctx.klt_level(which, l, wl, hl)
    for tag, args in (("which2", (2, 0, 16, 16)), ("which-1", (-1, 0, 16, 16)), ("level6", (0, 6, 1, 1)), ("level-1", (0, -1, 16, 16)),
                      ("w0", (0, 0, 0, 16)), ("h-3", (0, 0, 16, -3)), ("w_cap", (0, 1, CTX_W // 2 + 1, 16)), ("h_cap", (1, 0, 16, CTX_H + 1)),
                      ("last_level_cap", (0, 5, (CTX_W + 31) // 32 + 1, 1))):
        codes[tag] = lib.vo_test_klt_level(ctx._h, *args, p(buf))
    codes["null_out"] = lib.vo_test_klt_level(ctx._h, 0, 0, 16, 16, None)
    codes["null_ctx"] = lib.vo_test_klt_level(None, 0, 0, 16, 16, p(buf))
    codes["untouched"] = bool((buf == 0xEE).all())
    codes["ok"] = lib.vo_test_klt_level(ctx._h, 1, 5, (CTX_W + 31) // 32, (CTX_H + 31) // 32, p(buf))
    try:
        ctx.klt_level(0, 9, 4, 4)
        codes["wrapper"] = 0
    except _native.VoError as e:
        codes["wrapper"] = e.code
    ctx.close()
    np.savez(path, **out)
    print("KLT-DEF-RESULT " + json.dumps(codes))


# ------------------------------------------------------------------------------------------------ in the test process
_RUN = []


@pytest.fixture(scope="module")
def device():
    """every device call of the module, made once by one child process -> (arrays by name, the export's return codes)"""
    if not _RUN:
        hooks = os.path.join(ROOT, "openvo_amd", "libvo355_hooks.so")
        assert os.path.exists(hooks), "build the test-only library first (__graft_entry__.build())"
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "klt_def_device.npz")
            try:
                r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_klt_definitions as t; t._device_body(%r)" % path], cwd=ROOT,
                                   env=dict(os.environ, VO355_LIB=hooks), capture_output=True, text=True, timeout=240)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("KLT-DEF-RESULT ")]
                if r.returncode == 0 and lines:
                    z = np.load(path)
                    _RUN.append(({k: z[k] for k in z.files}, json.loads(lines[-1][len("KLT-DEF-RESULT "):])))
                else:
                    _RUN.append("the child ended with %d: %s" % (r.returncode, r.stdout[-3000:] + r.stderr[-3000:]))
            except subprocess.TimeoutExpired:
                _RUN.append("the child ran into its time limit")          # (it is not started again)
    assert not isinstance(_RUN[0], str), _RUN[0]
    return _RUN[0]


def _got(device, case):
    return tuple(device[0]["%s|%s" % (case["name"], k)] for k in ("xy", "st", "it"))


def _fig(r):
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items() if not isinstance(v, np.ndarray)}


PYR_NAMES = [c["name"] for c in DC.cases() if _levels_of(c)]


@pytest.mark.parametrize("name", PYR_NAMES)
def test_pyramid_levels_equal_the_definition(device, name):
    """both images (white noise and the 0 / 255 pattern of ties on the pyramid shapes), every level: equal, pixel by pixel"""
    case = DC.by_name(name)
    h, w = case["a"].shape
    lv = _levels_of(case)
    if case["kind"] == "pyr" and w >= 4 and h >= 2:
        assert DC.tie_share(case["b"]) >= 0.01                        # (on the definition alone)
    for which, img in enumerate((case["a"], case["b"])):
        got = [device[0]["%s|L%d%d" % (name, which, l)] for l in range(lv)]
        assert [g.shape[::-1] for g in got] == DC.level_sizes(w, h, lv)
        assert np.array_equal(got[0], img)
        bad = D.check_pyramid(got, img)
        assert bad == 0, "%s image %d: %d pixels differ from the definition" % (name, which, bad)
    print("%s: %d levels of 2 images equal" % (name, lv))


HELD = [c["name"] for c in DC.cases() if c["kind"] != "pyr"]


@pytest.mark.parametrize("name", HELD)
def test_device_is_held_by_the_definition(device, name):
    """one step under its derived bound; statuses wherever the definition decides; positions within TAU under the caps"""
    case = DC.by_name(name)
    cap = DC.caps(case)                                               # on the definition alone, before the result is looked at
    why, r = DC.hold(case, _got(device, case))
    print("%s: caps %s figures %s" % (name, cap, _fig(r)))
    assert not why, why


BITWISE = [c["name"] for c in DC.cases() if c["kind"] in ("narrow", "extreme")]


@pytest.mark.parametrize("name", BITWISE)
def test_narrow_and_extreme_cases_equal_the_restatement_bit_for_bit(device, name):
    """images narrower than the window (every read clamped, nothing refused, LOST at +-win) and sums beyond 2^31 / 2^32 (int32 lane
    sums, the int64 wave sum, the template packed as int16 pairs): positions, status bytes and iteration counts"""
    case = DC.by_name(name)
    want = K.track(case["a"], case["b"], case["xy"], **case["prm"])
    for g, w, what in zip(_got(device, case), want, ("xy", "status", "iters")):
        assert C.same_bits(g, w), "%s: %s differs: %r != %r" % (name, what, g, w)


def test_the_export_refuses_what_it_must(device):
    codes = device[1]
    print(codes)
    assert codes["fresh"] == VO_E_STATE
    for tag in ("which2", "which-1", "level6", "level-1", "w0", "h-3", "null_out", "null_ctx"):
        assert codes[tag] == VO_E_ARG, tag
    for tag in ("w_cap", "h_cap", "last_level_cap"):
        assert codes[tag] == VO_E_CAP, tag
    assert codes["untouched"] and codes["ok"] == 0 and codes["wrapper"] == VO_E_ARG
