"""ctypes binding of libvo355.so (C ABI: include/vo355.h).

The library is built in-tree by `build_native()` (hipcc, gfx950).  There is no CPU fallback:
creating a `Context` without a usable HIP device raises `VoError`.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VO355_LIB") or os.path.join(_HERE, "libvo355.so")   # VO355_LIB: A/B another build of the same ABI
_CSRC = os.path.join(_HERE, "csrc")

VO_NUM_SLOTS = 28
VO_NUM_HOST_STAGE = 20
VO_NUM_MONO_ASYNC = 5
VO_NUM_POSE_ASYNC = 8
VO_NUM_MAPS = 4
SCHED_DIAG, SCHED_DIAG_RAGGED, SCHED_UNFUSED = 1, 2, 3
SCHED_VERT, SCHED_VERT_RAGGED = 4, 5             # mode 2 (MODE_SGBM_3WAY): the vertical sweep in the diagonal sweep's place
COST_BT, COST_CENSUS = 0, 1                      # vo_set_sgbm_cost: the matching cost in front of the aggregation
T_STAGES = ("upload", "sgbm_cost", "sgbm_agg", "sgbm_wta", "sgbm_post", "orb", "match", "pose", "knn")

# every symbol include/vo355.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "vo_create", "vo_destroy", "vo_last_error", "vo_device_name", "vo_synchronize", "vo_set_engines",
    "vo_set_rectify_maps", "vo_set_sgbm", "vo_set_Q", "vo_set_roi", "vo_upload_pair",
    "vo_stage_pairs_alloc", "vo_stage_pair", "vo_load_staged_pair", "vo_prefetch_staged_pair",
    "vo_set_lookahead_orb", "vo_prefetch_pair",
    "vo_sgbm_compute", "vo_sgbm_compute_host", "vo_download_disparity_f32", "vo_download_xyz",
    "vo_download_left", "vo_download_right", "vo_cvt_bgr2gray", "vo_remap", "vo_reproject_to_3d",
    "vo_orb_detect_and_compute", "vo_orb_detect_and_compute_host", "vo_slot_num_keypoints", "vo_download_keypoints",
    "vo_bf_knn2_hamming", "vo_ratio_filter", "vo_points3d_at", "vo_bilinear_at", "vo_point_clouds",
    "vo_pose_pair", "vo_pose_pair_begin", "vo_pose_pair_end", "vo_ransac_essential", "vo_ransac_essential5", "vo_ransac_pnp", "vo_umeyama", "vo_rigid_clique", "vo_rodrigues", "vo_enable_timing", "vo_get_timings",
    "vo_sgbm_last_geometry", "vo_host_stage_pair", "vo_host_stage_fetch", "vo_prefetch_host_staged", "vo_lookahead_depth", "vo_lookahead_drop", "vo_sgbm_last_schedule", "vo_measure_copy", "vo_measure_knn", "vo_shader_clock", "vo_sgbm_sweep_status", "vo_sgbm_sweep_stats",
    "vo_upload_mono", "vo_prefetch_staged_mono", "vo_mono_pair", "vo_mono_pair_begin", "vo_mono_pair_end", "vo_slot_ready", "vo_host_stage_begin", "vo_host_stage_wait",
    "vo_device_count", "vo_mgpu_unique_id", "vo_mgpu_create", "vo_mgpu_destroy", "vo_mgpu_info", "vo_mgpu_last_error",
    "vo_mgpu_gather_poses", "vo_mgpu_all_gather_f64", "vo_mgpu_all_reduce_max_f64",
    "vo_bf_knn2_hamming_mutual", "vo_point_clouds_ex", "vo_pose_pair_ex", "vo_pose_pair_begin_ex", "vo_mono_pair_ex",
    "vo_mono_pair_begin_ex", "vo_measure_knn_ex",
    "vo_set_sweep_group", "vo_lookahead_flush", "vo_sweep_group_stats",
    "vo_pnp_pair", "vo_pnp_pair_begin", "vo_pnp_pair_end",
    "vo_recover_pose", "vo_mono_pose_pair", "vo_mono_pose_pair_begin", "vo_mono_pose_pair_end", "vo_download_mono_depth",
    "vo_set_match_window", "vo_clear_match_window", "vo_bf_knn2_hamming_window",
    "vo_sparse_stereo", "vo_download_keypoint_depth", "vo_sparse_match_host",
    "vo_sparse_pair_host", "vo_prefetch_pair_sparse", "vo_prefetch_host_staged_sparse", "vo_prefetch_staged_pair_sparse",
    "vo_set_sparse_assoc", "vo_download_keypoint_rdesc", "vo_sparse_pair_host_ex", "vo_set_match_loop", "vo_clear_match_loop",
    "vo_get_stage_timeline",
    "vo_map_create", "vo_map_destroy", "vo_map_reset", "vo_map_view", "vo_map_update", "vo_map_download",
    "vo_track_map",
    "vo_pnp_pair_lo", "vo_pnp_pair_begin_lo", "vo_pnp_pair_end_lo", "vo_track_map_lo",
    "vo_klt_track_host", "vo_klt_track", "vo_klt_pnp_pair", "vo_klt_pnp_pair_begin", "vo_klt_pnp_pair_end",
    "vo_set_sgbm_cost", "vo_get_sgbm_cost", "vo_sgbm_cost_volume",
    "vo_direct_align", "vo_direct_align_ab", "vo_direct_align_kp",
]


class VoError(RuntimeError):
    """Raised for any non-zero status of the native library (code in .code)."""

    def __init__(self, code, msg):
        super().__init__("libvo355 error %d: %s" % (code, msg))
        self.code = code


class SweepTimeout(VoError):
    """VO_E_SWEEP: the disparity a result depends on is undefined (a strip hand-off of that pair's aggregation sweep gave up
    waiting, e.g. on an oversubscribed GPU).  Nothing computed from it is handed out; the pair can be submitted again."""


VO_E_SWEEP = -6


class MonoPose(ctypes.Structure):
    """vo_mono_pose of include/vo355.h: the record of vo_recover_pose and of a monocular pose step."""
    _fields_ = [("M", ctypes.c_int32), ("best_iter", ctypes.c_int32), ("best_count", ctypes.c_int32), ("winner", ctypes.c_int32),
                ("n_depth", ctypes.c_int32), ("n_shared", ctypes.c_int32), ("flags", ctypes.c_int32), ("serial", ctypes.c_uint32),
                ("votes4", ctypes.c_int32 * 4), ("E", ctypes.c_double * 9), ("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3),
                ("scale_rel", ctypes.c_double)]

    def as_dict(self):
        return dict(matches=int(self.M), best_iter=int(self.best_iter), best_count=int(self.best_count), winner=int(self.winner),
                    n_depth=int(self.n_depth), n_shared=int(self.n_shared), flags=int(self.flags), serial=int(self.serial),
                    votes4=np.array(self.votes4[:], np.int32), E=np.array(self.E[:], np.float64).reshape(3, 3),
                    R=np.array(self.R[:], np.float64).reshape(3, 3), t=np.array(self.t[:], np.float64), scale_rel=float(self.scale_rel))


class MapTrackRec(ctypes.Structure):
    """vo_track_map_rec of include/vo355.h: the record of the fused map step."""
    _fields_ = [("decision", ctypes.c_int32), ("map_n", ctypes.c_int32), ("vis", ctypes.c_int32), ("update_flags", ctypes.c_int32),
                ("M", ctypes.c_int32), ("n", ctypes.c_int32), ("best_iter", ctypes.c_int32), ("best_count", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("rstatus", ctypes.c_int32), ("rsteps", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("counts6", ctypes.c_int32 * 6), ("pad2", ctypes.c_int32 * 2),
                ("Rt", ctypes.c_double * 12), ("Rtr", ctypes.c_double * 12), ("c_T_w", ctypes.c_double * 12), ("w_T_c", ctypes.c_double * 12)]

    def as_dict(self):
        m34 = lambda a: np.array(a[:], np.float64).reshape(3, 4)                     # noqa: E731
        return dict(decision=int(self.decision), view=np.array([self.map_n, self.vis], np.int32), update_flags=int(self.update_flags),
                    matches=int(self.M), n=int(self.n), best_iter=int(self.best_iter), best_count=int(self.best_count), flags=int(self.flags),
                    refine_status=int(self.rstatus), refine_steps=int(self.rsteps), update=np.array(self.counts6[:], np.int32),
                    Rt=m34(self.Rt), Rt_refined=m34(self.Rtr), c_T_w=m34(self.c_T_w), w_T_c=m34(self.w_T_c))


DIRECT_MAX_LEVELS = 4     # VO_DIRECT_MAX_LEVELS


class DirectLevel(ctypes.Structure):
    """vo_direct_level of include/vo355.h"""
    _fields_ = [("s", ctypes.c_int32), ("selected", ctypes.c_int32), ("n_first", ctypes.c_int32), ("n_last", ctypes.c_int32),
                ("wr2_first", ctypes.c_double), ("wr2_last", ctypes.c_double)]


class DirectRec(ctypes.Structure):
    """vo_direct_rec of include/vo355.h: the record of the dense direct alignment."""
    _fields_ = [("status", ctypes.c_int32), ("iters_done", ctypes.c_int32), ("levels", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("lv", DirectLevel * DIRECT_MAX_LEVELS), ("Rt", ctypes.c_double * 12), ("sums", ctypes.c_double * 27),
                ("count", ctypes.c_double), ("wr2", ctypes.c_double)]

    def as_dict(self):
        n = int(self.levels)
        sums = np.array(self.sums[:], np.float64)
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = sums[:21]                # packed upper triangle in row order
        H = H + np.triu(H, 1).T
        lv = [self.lv[l] for l in range(n)]
        return dict(status=int(self.status), iters_done=int(self.iters_done),
                    s=np.array([v.s for v in lv], np.int32), selected=np.array([v.selected for v in lv], np.int32),
                    n_first=np.array([v.n_first for v in lv], np.int32), n_last=np.array([v.n_last for v in lv], np.int32),
                    wr2_first=np.array([v.wr2_first for v in lv], np.float64), wr2_last=np.array([v.wr2_last for v in lv], np.float64),
                    Rt=np.array(self.Rt[:], np.float64).reshape(3, 4), sums=sums, information=H, g=sums[21:].copy(),
                    count=int(self.count), wr2=float(self.wr2))


class DirectAbRec(ctypes.Structure):
    """vo_direct_ab_rec of include/vo355.h: the record of the dense direct alignment with the affine brightness term."""
    _fields_ = [("status", ctypes.c_int32), ("iters_done", ctypes.c_int32), ("levels", ctypes.c_int32), ("unknowns", ctypes.c_int32),
                ("lv", DirectLevel * DIRECT_MAX_LEVELS), ("Rt", ctypes.c_double * 12), ("k", ctypes.c_double), ("m", ctypes.c_double),
                ("sums", ctypes.c_double * 44), ("count", ctypes.c_double), ("wr2", ctypes.c_double)]

    def as_dict(self):
        n, nu = int(self.levels), int(self.unknowns)
        if nu not in (6, 8):
            raise ValueError("vo_direct_ab_rec: unknowns is %d, neither 6 nor 8" % nu)
        nh = nu * (nu + 1) // 2
        sums = np.array(self.sums[:], np.float64)
        full = np.zeros((8, 8))
        tri = np.zeros((nu, nu))
        tri[np.triu_indices(nu)] = sums[:nh]             # packed upper triangle in row order
        full[:nu, :nu] = tri + np.triu(tri, 1).T
        g = np.zeros(8)
        g[:nu] = sums[nh:nh + nu]
        info = full[:6, :6].copy()
        if nu == 8:                                      # the pose information marginalised over the brightness
            info = info - full[:6, 6:] @ np.linalg.solve(full[6:, 6:], full[6:, :6])
            info = 0.5 * (info + info.T)
        lv = [self.lv[l] for l in range(n)]
        return dict(status=int(self.status), iters_done=int(self.iters_done),
                    s=np.array([v.s for v in lv], np.int32), selected=np.array([v.selected for v in lv], np.int32),
                    n_first=np.array([v.n_first for v in lv], np.int32), n_last=np.array([v.n_last for v in lv], np.int32),
                    wr2_first=np.array([v.wr2_first for v in lv], np.float64), wr2_last=np.array([v.wr2_last for v in lv], np.float64),
                    Rt=np.array(self.Rt[:], np.float64).reshape(3, 4), gain=float(self.k), offset=float(self.m), unknowns=nu, sums=sums,
                    information_full=full, information=info, g=g, count=int(self.count), wr2=float(self.wr2))


MAP_TRACK_MAX = 3800     # VO_MAP_TRACK_MAX: the largest map the fused map step takes
MAP_DECISIONS = {0: "", 1: None, 2: "matches", 3: "matches", 4: "outlier", 5: "nan", 6: "bigdist", 7: "bigrot"}     # decision -> skip_cause (None: none set)


def _image(img):
    """(img, channels) as a C-contiguous uint8 array: HxW or HxWx3 (HxWx1 is squeezed); anything else -- e.g. HxWx4 -- is
    refused here, before a pointer reaches native code that would read w*h*channels bytes from it."""
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("an image must be HxW or HxWx3 (got shape %s)" % (a.shape,))
    return _c(a, np.uint8), (3 if a.ndim == 3 else 1)


def _image_pair(left, right):
    """(left, right, channels): two images of one shape, each under the rule of _image."""
    (left, ch), (right, _) = _image(left), _image(right)
    if left.shape != right.shape:
        raise ValueError("left/right shapes differ")
    return left, right, ch


def csrc_digest():
    """sha256 over the kernel sources (csrc/*.hip, *.inc, *.h + the public header), in name order: stamps a profile with the code it
    was taken from (tools/profile_round.sh) and lets bench.py say when the committed counters describe other kernels."""
    import hashlib
    h = hashlib.sha256()
    names = sorted(f for f in os.listdir(_CSRC) if f.endswith((".hip", ".inc", ".h")))
    for path in [os.path.join(_CSRC, f) for f in names] + [os.path.join(_HERE, "..", "include", "vo355.h")]:
        h.update(os.path.basename(path).encode() + b"\0")
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def build_native(force=False):
    """Compile openvo_amd/csrc/*.hip for gfx950 into openvo_amd/libvo355.so."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h", ".inc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "vo355.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "vo_orb_pattern.inc"))
    newest = max(os.path.getmtime(s) for s in srcs)
    hooks = os.path.join(_HERE, "libvo355_hooks.so")       # test-only build with the failure-injection hook (tests load it by path)
    built = os.path.join(_HERE, "libvo355.so")
    if force or any(not os.path.exists(q) or os.path.getmtime(q) < newest for q in (built, hooks)):
        subprocess.check_call(["make", "-C", _CSRC, "-j4", "all"] + (["-B"] if force else []),
                              stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    """Load libvo355.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvo355.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        L.vo_last_error.restype = ctypes.c_char_p
        L.vo_last_error.argtypes = [ctypes.c_void_p]
        L.vo_destroy.restype = None
        L.vo_destroy.argtypes = [ctypes.c_void_p]
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.vo_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(vp)]
        L.vo_set_engines.argtypes = [vp, ci]
        L.vo_device_name.argtypes = [vp, ctypes.c_char_p, ci]
        L.vo_synchronize.argtypes = [vp]
        L.vo_set_rectify_maps.argtypes = [vp, ci, vp, vp, ci, ci]
        L.vo_set_sgbm.argtypes = [vp] + [ci] * 11
        L.vo_set_Q.argtypes = [vp, vp]
        L.vo_set_roi.argtypes = [vp, ci, ci, ci, ci]
        L.vo_upload_pair.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci]
        L.vo_stage_pairs_alloc.argtypes = [vp, ci, ci, ci, ci]
        L.vo_stage_pair.argtypes = [vp, ci, vp, vp]
        L.vo_load_staged_pair.argtypes = [vp, ci, ci, ci]
        L.vo_prefetch_staged_pair.argtypes = [vp, ci, ci, ci]
        L.vo_set_lookahead_orb.argtypes = [vp, ci, ci, ci, ci, ci]
        L.vo_prefetch_pair.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci]
        L.vo_sgbm_compute.argtypes = [vp, ci, vp]
        L.vo_sgbm_compute_host.argtypes = [vp, vp, vp, ci, ci, vp]
        for f in (L.vo_download_disparity_f32, L.vo_download_xyz, L.vo_download_left, L.vo_download_right):
            f.argtypes = [vp, ci, vp]
        L.vo_cvt_bgr2gray.argtypes = [vp, vp, ci, ci, vp]
        L.vo_remap.argtypes = [vp, ci, vp, ci, ci, vp]
        L.vo_reproject_to_3d.argtypes = [vp, vp, ci, ci, vp, vp]
        L.vo_orb_detect_and_compute.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp]
        L.vo_orb_detect_and_compute_host.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp]
        L.vo_slot_num_keypoints.argtypes = [vp, ci, vp]
        L.vo_download_keypoints.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, vp]
        L.vo_bf_knn2_hamming.argtypes = [vp, vp, ci, vp, ci, vp, vp]
        L.vo_ratio_filter.argtypes = [vp, vp, ci, cd, vp, vp, vp]
        L.vo_points3d_at.argtypes = [vp, ci, vp, ci, vp, vp]
        L.vo_bilinear_at.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp]
        L.vo_point_clouds.argtypes = [vp, ci, ci, cd, vp, vp, vp, vp, vp, vp, ci, vp]
        L.vo_pose_pair.argtypes = [vp, ci, ci, cd, ci, cd, cd, vp, vp, vp, vp]
        L.vo_pose_pair_begin.argtypes = [vp, ci, ci, cd, ci, cd, cd, vp]
        L.vo_pose_pair_end.argtypes = [vp, ci, vp, vp, vp, vp]
        L.vo_ransac_essential.argtypes = [vp, vp, vp, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, vp, vp, vp, vp]
        L.vo_ransac_essential5.argtypes = L.vo_ransac_essential.argtypes
        L.vo_ransac_pnp.argtypes = [vp, vp, vp, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, vp, vp, vp, vp]
        L.vo_umeyama.argtypes = [vp, vp, vp, ci, ci, vp, vp]
        L.vo_rigid_clique.argtypes = [vp, vp, vp, ci, cd, vp]
        L.vo_rodrigues.argtypes = [vp, vp]
        L.vo_enable_timing.argtypes = [vp, ci]
        L.vo_get_timings.argtypes = [vp, vp, vp, ci]
        L.vo_sgbm_last_geometry.argtypes = [vp, vp, vp]
        L.vo_sgbm_sweep_status.argtypes = [vp, vp]
        L.vo_lookahead_depth.argtypes = [vp, vp]
        L.vo_host_stage_pair.argtypes = [vp, ci, vp, vp, ci, ci, ci]
        L.vo_host_stage_fetch.argtypes = [vp, ci, vp, vp, ci, ci, ci]
        L.vo_prefetch_host_staged.argtypes = [vp, ci, ci, ci, ci, ci, ci]
        L.vo_lookahead_drop.argtypes = [vp, ci]
        L.vo_sgbm_last_schedule.argtypes = [vp, vp]
        L.vo_sgbm_sweep_stats.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int]
        L.vo_measure_copy.argtypes = [vp, ctypes.c_int64, ci, ci, vp]
        L.vo_shader_clock.argtypes = [vp, ci, vp]
        L.vo_measure_knn.argtypes = [vp, ci, ci, ci, vp]
        L.vo_upload_mono.argtypes = [vp, ci, vp, ci, ci, ci]
        L.vo_prefetch_staged_mono.argtypes = [vp, ci, ci, ci]
        L.vo_mono_pair.argtypes = [vp, ci, ci, cd, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, ci]
        L.vo_slot_ready.argtypes = [vp, ci, vp]
        L.vo_host_stage_begin.argtypes = [vp, ci, vp, vp, ci, ci, ci]
        L.vo_host_stage_wait.argtypes = [vp, ci]
        L.vo_mono_pair_begin.argtypes = [vp, ci, ci, cd, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, ci, vp]
        L.vo_mono_pair_end.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci]
        L.vo_bf_knn2_hamming_mutual.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp]
        L.vo_point_clouds_ex.argtypes = [vp, ci, ci, cd, ci, vp, vp, vp, vp, vp, vp, ci, vp]
        L.vo_pose_pair_ex.argtypes = [vp, ci, ci, cd, ci, ci, cd, cd, vp, vp, vp, vp]
        L.vo_pose_pair_begin_ex.argtypes = [vp, ci, ci, cd, ci, ci, cd, cd, vp]
        L.vo_mono_pair_ex.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, ci]
        L.vo_mono_pair_begin_ex.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, ci, vp]
        L.vo_measure_knn_ex.argtypes = [vp, ci, ci, ci, ci, vp]
        L.vo_set_match_window.argtypes = [vp, ctypes.c_float, ctypes.c_float]
        L.vo_clear_match_window.argtypes = [vp]
        L.vo_bf_knn2_hamming_window.argtypes = [vp, vp, ci, vp, ci, vp, vp, ctypes.c_float, ctypes.c_float, ci, vp, vp, vp, vp]
        if hasattr(L, "vo_sparse_stereo"):          # (an older build has no sparse stereo depth)
            cf = ctypes.c_float
            for name, proto in (("vo_sparse_stereo", [vp, ci, ci, cf, cf, cf, ci, vp]),
                                ("vo_download_keypoint_depth", [vp, ci, vp, vp, ci, vp]),
                                ("vo_sparse_match_host", [vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, cf, cf, cf, ci, vp, vp])):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_prefetch_pair_sparse"):   # (likewise: an older build starts no sparse pair ahead)
            cf = ctypes.c_float
            req = [ci, cf, cf, cf, ci]
            for name, proto in (("vo_prefetch_pair_sparse", [vp, ci, vp, vp, ci, ci, ci, ci] + req),
                                ("vo_prefetch_host_staged_sparse", [vp, ci, ci, ci, ci, ci, ci] + req),
                                ("vo_prefetch_staged_pair_sparse", [vp, ci, ci, ci] + req),
                                ("vo_sparse_pair_host", [vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, cf, cf, cf, ci, vp, ci, ci] + [vp] * 8)):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_set_sparse_assoc"):       # (likewise: an older build has no association tests)
            cf = ctypes.c_float
            for name, proto in (("vo_set_sparse_assoc", [vp, ci, cf]), ("vo_download_keypoint_rdesc", [vp, ci, vp, ci, vp]),
                                ("vo_set_match_loop", [vp, ci]), ("vo_clear_match_loop", [vp]),
                                ("vo_sparse_pair_host_ex", [vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, cf, cf, cf, ci, ci, cf, vp, ci, ci] + [vp] * 9)):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_pnp_pair"):               # (likewise: an older build has no fused PnP step)
            L.vo_pnp_pair.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci]
            L.vo_pnp_pair_begin.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, ctypes.c_uint32, ci, ci, vp]
            L.vo_pnp_pair_end.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci]
        if hasattr(L, "vo_recover_pose"):           # (likewise: an older build has no pose recovery on the device)
            cu = ctypes.c_uint32
            L.vo_recover_pose.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, vp, cd, vp, vp, vp, vp]
            L.vo_mono_pose_pair.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, cu, ci, cu, cd, vp]
            L.vo_mono_pose_pair_begin.argtypes = [vp, ci, ci, cd, ci, vp, ci, ctypes.c_float, cu, ci, cu, cd, vp, vp]
            L.vo_mono_pose_pair_end.argtypes = [vp, ci, vp]
            L.vo_download_mono_depth.argtypes = [vp, ci, vp, vp]
        if hasattr(L, "vo_get_stage_timeline"):     # (likewise: an older build has no stage timeline)
            L.vo_get_stage_timeline.argtypes = [vp, ci, vp, vp, vp, vp, vp]
        if hasattr(L, "vo_lookahead_flush"):        # (an older build of the ABI loaded through VO355_LIB for an A/B run has no sweep groups)
            L.vo_set_sweep_group.argtypes = [vp, ci]
            L.vo_lookahead_flush.argtypes = [vp]
            L.vo_sweep_group_stats.argtypes = [vp, vp, vp]
        if hasattr(L, "vo_map_create"):             # (likewise: an older build has no landmark map)
            for name, proto in (("vo_map_create", [vp, ci, vp]), ("vo_map_destroy", [vp, ci]), ("vo_map_reset", [vp, ci]),
                                ("vo_map_view", [vp, ci, vp, vp, ctypes.c_float, ci, ci, vp]),
                                ("vo_map_update", [vp, ci, ci, vp, ci, ci, ci, vp, vp, vp, ci, vp]),
                                ("vo_map_download", [vp, ci, vp, vp, vp, vp, vp, ci, vp])):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_track_map"):              # (likewise: an older build has no fused map step)
            cf, cu = ctypes.c_float, ctypes.c_uint32
            for name, proto in (("vo_track_map", [vp, ci, ci, ci, vp, vp, cf, cd, ci, ci, cf, cu, ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, ci]),):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_pnp_pair_lo"):            # (likewise: an older build has no local-optimisation rounds)
            cf, cu = ctypes.c_float, ctypes.c_uint32
            for name, proto in (("vo_pnp_pair_lo", [vp, ci, ci, cd, ci, vp, ci, cf, cu, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
                                ("vo_pnp_pair_begin_lo", [vp, ci, ci, cd, ci, vp, ci, cf, cu, ci, ci, ci, vp]),
                                ("vo_pnp_pair_end_lo", [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]),
                                ("vo_track_map_lo", [vp, ci, ci, ci, vp, vp, cf, cd, ci, ci, cf, cu, ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, ci, ci])):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_klt_track"):              # (likewise: an older build has no Lucas-Kanade tracker)
            for name, proto in (("vo_klt_track_host", [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, cd, cd, cd, vp, vp, vp]),
                                ("vo_klt_track", [vp, ci, ci, ci, ci, ci, cd, cd, cd, vp, vp, vp, ci, vp])):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_klt_pnp_pair"):           # (likewise: an older build has no fused Lucas-Kanade PnP step)
            cf, cu = ctypes.c_float, ctypes.c_uint32
            front = [vp, ci, ci, ci, ci, ci, cd, cd, cd, vp, ci, cf, cu, ci, ci]
            for name, proto in (("vo_klt_pnp_pair", front + [vp] * 9 + [ci]), ("vo_klt_pnp_pair_begin", front + [ci, vp]),
                                ("vo_klt_pnp_pair_end", [vp, ci] + [vp] * 9 + [ci])):
                getattr(L, name).argtypes = proto
        if hasattr(L, "vo_set_sgbm_cost"):          # (likewise: an older build has the BT cost alone)
            for name, proto in (("vo_set_sgbm_cost", [vp, ci, ci, ci]), ("vo_get_sgbm_cost", [vp, vp, vp, vp]),
                                ("vo_sgbm_cost_volume", [vp, vp, ctypes.c_size_t])):
                getattr(L, name).argtypes = proto
        for name in ("vo_direct_align", "vo_direct_align_ab"):      # (likewise: an older build has no dense direct alignment, or no affine term)
            if hasattr(L, name):
                getattr(L, name).argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ci, cd, cd, cd, cd, ci, vp]
        for name in ("vo_direct_align_kp",):        # (likewise: an older build has no patch alignment)
            if hasattr(L, name):
                getattr(L, name).argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ci, cd, cd, ci, vp]
        plant = getattr(L, "vo_test_plant_dense_pair", None)     # (only the test-only build, libvo355_hooks.so, exports it)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, vp]
        plant = getattr(L, "vo_test_plant_keypoints", None)      # (only the test-only build, libvo355_hooks.so, exports it)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, vp, vp, vp, vp]
        plant = getattr(L, "vo_test_plant_dense", None)          # (likewise)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp]
        plant = getattr(L, "vo_test_plant_map", None)            # (likewise)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp]
        plant = getattr(L, "vo_test_peek_view", None)            # (likewise)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        plant = getattr(L, "vo_test_klt_level", None)            # (likewise)
        if plant is not None:
            plant.argtypes = [vp, ci, ci, ci, ci, vp]
        L.vo_device_count.argtypes = [vp]
        L.vo_mgpu_unique_id.argtypes = [vp]
        L.vo_mgpu_create.argtypes = [ci, ci, ci, vp, vp]
        L.vo_mgpu_destroy.restype = None
        L.vo_mgpu_destroy.argtypes = [vp]
        L.vo_mgpu_last_error.restype = ctypes.c_char_p
        L.vo_mgpu_last_error.argtypes = [vp]
        L.vo_mgpu_gather_poses.argtypes = [vp, vp, ci, vp]
        L.vo_mgpu_all_gather_f64.argtypes = [vp, vp, ci, vp]
        L.vo_mgpu_all_reduce_max_f64.argtypes = [vp, vp, ci]
        _lib = L
    return _lib


VO_MATCH_CROSSCHECK = 1
VO_MATCH_WINDOW = 2
VO_MATCH_LOOP = 4


def loop_threshold(loop, what="loop"):
    """None | int 0 .. 256 -> None | int; ValueError for anything else"""
    if loop is None:
        return None
    if isinstance(loop, (bool, np.bool_)) or not isinstance(loop, (int, np.integer)) or not 0 <= loop <= 256:
        raise ValueError("%s is None or an int in 0 .. 256, not %r" % (what, loop))
    return int(loop)


def _flags(cross_check):
    """match_flags of the _ex entries"""
    return VO_MATCH_CROSSCHECK if cross_check else 0


def window_radii(window, what="window"):
    """None | number (both radii) | (rx, ry) -> None | (rx, ry) as the float32 values the kernel compares with; ValueError for
    anything else, negative or non-finite"""
    if window is None:
        return None
    try:
        if isinstance(window, (bool, str, bytes)):
            raise TypeError
        w = (window, window) if np.ndim(window) == 0 else tuple(window)
        if len(w) != 2:
            raise TypeError
        with np.errstate(over="ignore"):              # (too large for float32: inf, refused below)
            rx, ry = float(np.float32(w[0])), float(np.float32(w[1]))
    except (TypeError, ValueError):
        raise ValueError("%s is None, a radius or a pair (rx, ry) of pixels, not %r" % (what, window))
    if not (np.isfinite(rx) and np.isfinite(ry) and rx >= 0 and ry >= 0):
        raise ValueError("%s: the radii must be finite and >= 0, not %r" % (what, window))
    return rx, ry


VO_SPARSE_MUTUAL = 1
VO_SPARSE_RATIO = 2


def sparse_assoc_state(mutual=False, ratio=None):
    """(mutual, ratio) -> (flags, float32 ratio) as vo_set_sparse_assoc takes them; ValueError for a mutual that is no bool or a
    ratio that is neither None nor a number with 0 < ratio <= 1"""
    if not isinstance(mutual, (bool, np.bool_)):
        raise ValueError("mutual is True or False, not %r" % (mutual,))
    flags = VO_SPARSE_MUTUAL if mutual else 0
    if ratio is None:
        return flags, 0.0
    try:
        if isinstance(ratio, (bool, str, bytes)) or np.ndim(ratio) != 0:
            raise TypeError
        r = float(np.float32(ratio))
    except (TypeError, ValueError):
        raise ValueError("the association ratio is None or a number with 0 < ratio <= 1, not %r" % (ratio,))
    if not (0.0 < r <= 1.0):
        raise ValueError("the association ratio is None or a number with 0 < ratio <= 1, not %r" % (ratio,))
    return flags | VO_SPARSE_RATIO, r


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


class Context:
    """One device context (one HIP stream).  Not thread-safe: one per thread / per GPU."""

    def __init__(self, device=0, max_w=1280, max_h=720, max_disp=128, max_kp=2000, engines=None):
        """engines: how many look-ahead engines the context may use (None: the library's default of 16, or VO_ENGINES) -- each
        owns a stream and, from its first use on, a full SGBM + ORB workspace (0.95 GB at 1280x720 / D = 128)."""
        self._lib = lib()
        h = ctypes.c_void_p()
        rc = self._lib.vo_create(int(device), int(max_w), int(max_h), int(max_disp), int(max_kp), ctypes.byref(h))
        if rc != 0:
            raise VoError(rc, (self._lib.vo_last_error(None) or b"").decode())
        self._h = h
        if engines is not None:
            if int(engines) < 1:
                self.close()
                raise ValueError("engines must be >= 1")
            self.set_engines(engines)
        self._la_orb = None
        self._window = None          # the match window this wrapper last set in the context
        self._loop = None            # ... and the threshold of the loop check
        self._sparse_assoc = (0, 0.0)    # ... and the association tests of the sparse chain (the context starts with none)
        self.device, self.max_w, self.max_h, self.max_disp, self.max_kp = device, max_w, max_h, max_disp, max_kp
        self.kp_cap = max_kp * 2 + 1024

    def set_engines(self, n=0):
        """-> the number of look-ahead engines in effect (n <= 0 only asks)."""
        rc = self._lib.vo_set_engines(self._h, int(n))
        if rc < 0:
            raise VoError(rc, "vo_set_engines")
        return rc

    def set_sweep_group(self, n=0):
        """-> how many look-ahead pairs share one aggregation sweep launch (n <= 0 only asks; 1 = every pair on its own)."""
        if not hasattr(self._lib, "vo_set_sweep_group"):
            return 1
        rc = self._lib.vo_set_sweep_group(self._h, int(n))
        if rc < 0:
            raise VoError(rc, (self._lib.vo_last_error(self._h) or b"").decode())
        return rc

    def lookahead_flush(self):
        """No further look-ahead pair follows now: the pairs the library still collects for a shared sweep are started as they
        stand.  -> the sweep group size in force."""
        if not hasattr(self._lib, "vo_lookahead_flush"):
            return 1
        rc = self._lib.vo_lookahead_flush(self._h)
        if rc < 0:
            raise VoError(rc, (self._lib.vo_last_error(self._h) or b"").decode())
        return rc

    def sweep_group_stats(self):
        """-> {"full", "consumer", "flush", "other"}: sweep groups closed so far by cause, and "open": members of the open one."""
        closed, n_open = np.zeros(4, np.int64), ctypes.c_int(0)
        self._ck(self._lib.vo_sweep_group_stats(self._h, _p(closed), ctypes.byref(n_open)))
        return dict(zip(("full", "consumer", "flush", "other"), (int(v) for v in closed)), open=n_open.value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise (SweepTimeout if rc == VO_E_SWEEP else VoError)(rc, (self._lib.vo_last_error(self._h) or b"").decode())

    # ---- configuration
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._ck(self._lib.vo_device_name(self._h, buf, 256))
        return buf.value.decode()

    def synchronize(self):
        self._ck(self._lib.vo_synchronize(self._h))

    def set_rectify_maps(self, cam, map1, map2):
        map1, map2 = _c(map1, np.int16), _c(map2, np.uint16)
        h, w = map2.shape
        self._ck(self._lib.vo_set_rectify_maps(self._h, cam, _p(map1), _p(map2), w, h))

    _sgbm_band = (0, 0)

    def set_sgbm(self, p, mode=0):
        """The ten StereoSGBM parameters, the mode (p["mode"] where there is one) and the matching cost: p["cost"] (COST_BT where
        there is none: the dict is the whole truth at this level), p["censusWidth"] (9), p["censusHeight"] (7).  A refusal of
        either part leaves both as they were."""
        has_cost = hasattr(self._lib, "vo_set_sgbm_cost")            # (an older build loaded for an A/B run has the BT cost alone)
        if not has_cost and int(p.get("cost", COST_BT)) != COST_BT:
            raise VoError(-1, "this build of libvo355 has no vo_set_sgbm_cost: only the BT cost")
        before = self.sgbm_cost() if has_cost else None
        if has_cost:
            self.set_sgbm_cost(int(p.get("cost", COST_BT)), (int(p.get("censusWidth", 9)), int(p.get("censusHeight", 7))))
        try:
            self._ck(self._lib.vo_set_sgbm(self._h, *[int(p[k]) for k in (
                "minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap",
                "uniquenessRatio", "speckleWindowSize", "speckleRange")], int(p.get("mode", mode))))
        except VoError:
            if has_cost:
                self.set_sgbm_cost(*before)
            raise
        self._sgbm_band = (int(p["minDisparity"]), int(p["numDisparities"]))

    def set_sgbm_cost(self, cost, window=(9, 7)):
        """The matching cost of the SGBM front: COST_BT (OpenCV's, the default) or COST_CENSUS with a window (width, height) out of
        {3, 5, 7, 9} x {3, 5, 7}.  Persists across the native vo_set_sgbm; Context.set_sgbm applies its dict's keys on every call."""
        self._ck(self._lib.vo_set_sgbm_cost(self._h, int(cost), int(window[0]), int(window[1])))

    def sgbm_cost(self):
        """-> (cost, (width, height)) in force"""
        c, w, h = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self._lib.vo_get_sgbm_cost(self._h, ctypes.byref(c), ctypes.byref(w), ctypes.byref(h)))
        return c.value, (w.value, h.value)

    def sgbm_cost_volume(self, w, h):
        """C (block cost + P2) of the latest synchronous SGBM run on a w x h pair as int16 [h][W1][D], W1 the computed band's width"""
        minD, D = self._sgbm_band
        W1 = int(w) + min(minD, 0) - max(minD + D, 0)
        out = np.empty((int(h), max(W1, 0), D), np.int16)
        self._ck(self._lib.vo_sgbm_cost_volume(self._h, _p(out), out.size))
        return out

    def set_Q(self, Q):
        Q = _c(Q, np.float64)
        self._ck(self._lib.vo_set_Q(self._h, _p(Q)))

    def set_roi(self, x0, y0, x1, y1):
        self._ck(self._lib.vo_set_roi(self._h, int(x0), int(y0), int(x1), int(y1)))

    # ---- per pair
    def upload_pair(self, slot, left, right, preprocessed):
        left, right, ch = _image_pair(left, right)
        h, w = left.shape[:2]
        self._ck(self._lib.vo_upload_pair(self._h, slot, _p(left), _p(right), w, h, ch, int(bool(preprocessed))))
        return w, h

    def prefetch_pair(self, slot, left, right, preprocessed):
        """Look-ahead from host images: pinned staging + async upload + SGBM (+ ORB) on an engine."""
        left, right, ch = _image_pair(left, right)
        h, w = left.shape[:2]
        self._ck(self._lib.vo_prefetch_pair(self._h, slot, _p(left), _p(right), w, h, ch, int(bool(preprocessed))))
        return w, h

    @staticmethod
    def _sparse_req(nfeatures, min_disp, max_disp, row_tol, max_hamming):
        """the five trailing arguments of the vo_prefetch_*_sparse entries (vo_sparse_stereo's request)"""
        return int(nfeatures), float(min_disp), float(max_disp), float(row_tol), int(max_hamming)

    def prefetch_pair_sparse(self, slot, left, right, preprocessed, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75):
        """Look-ahead from host images with the sparse stereo chain in place of the SGBM: sparse_stereo(slot, the same request)
        then only waits and collects."""
        left, right, ch = _image_pair(left, right)
        h, w = left.shape[:2]
        self._ck(self._lib.vo_prefetch_pair_sparse(self._h, int(slot), _p(left), _p(right), w, h, ch, int(bool(preprocessed)),
                                                   *self._sparse_req(nfeatures, min_disp, max_disp, row_tol, max_hamming)))
        return w, h

    def prefetch_host_staged_sparse(self, slot, buf, w, h, ch, preprocessed, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75):
        self._ck(self._lib.vo_prefetch_host_staged_sparse(self._h, int(slot), int(buf), w, h, ch, int(bool(preprocessed)),
                                                          *self._sparse_req(nfeatures, min_disp, max_disp, row_tol, max_hamming)))
        return w, h

    def prefetch_staged_pair_sparse(self, slot, index, preprocessed, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75):
        self._ck(self._lib.vo_prefetch_staged_pair_sparse(self._h, int(slot), int(index), int(bool(preprocessed)),
                                                          *self._sparse_req(nfeatures, min_disp, max_disp, row_tol, max_hamming)))
        return self.staged_shape

    def host_stage_pair(self, buf, left, right):
        """Copy a host pair into pinned staging buffer `buf` (waits for that buffer's previous upload).  The one call that
        may run on a helper thread while another thread drives this context."""
        left, right, ch = _image_pair(left, right)
        h, w = left.shape[:2]
        rc = self._lib.vo_host_stage_pair(self._h, int(buf), _p(left), _p(right), w, h, ch)
        if rc != 0:
            raise VoError(rc, "vo_host_stage_pair failed")      # (the context's error string belongs to the driving thread)
        return w, h, ch

    def host_stage_begin(self, buf, left, right):
        """The same copy on the library's own staging thread: returns at once with (w, h, ch, keep) -- `keep` holds the two
        arrays, which must stay alive and untouched until prefetch_host_staged / host_stage_fetch / host_stage_wait on `buf`."""
        left, right, ch = _image_pair(left, right)
        h, w = left.shape[:2]
        self._ck(self._lib.vo_host_stage_begin(self._h, int(buf), _p(left), _p(right), w, h, ch))
        return w, h, ch, (left, right)

    def host_stage_wait(self, buf):
        self._ck(self._lib.vo_host_stage_wait(self._h, int(buf)))

    def host_stage_fetch(self, buf, w, h, ch):
        shape = (h, w, 3) if ch == 3 else (h, w)
        left, right = np.empty(shape, np.uint8), np.empty(shape, np.uint8)
        self._ck(self._lib.vo_host_stage_fetch(self._h, int(buf), _p(left), _p(right), w, h, ch))
        return left, right

    def prefetch_host_staged(self, slot, buf, w, h, ch, preprocessed):
        self._ck(self._lib.vo_prefetch_host_staged(self._h, slot, int(buf), w, h, ch, int(bool(preprocessed))))
        return w, h

    def stage_pairs(self, pairs):
        """Upload a list of (left, right) host pairs once; they stay resident in HBM."""
        l0, _, ch = _image_pair(*pairs[0])
        h, w = l0.shape[:2]
        self._ck(self._lib.vo_stage_pairs_alloc(self._h, len(pairs), w, h, ch))
        for i, (l, r) in enumerate(pairs):
            l, r, _ = _image_pair(l, r)
            if l.shape != l0.shape:
                raise ValueError("all staged pairs must share one shape")
            self._ck(self._lib.vo_stage_pair(self._h, i, _p(l), _p(r)))
        self.staged_shape = (w, h)

    def load_staged_pair(self, slot, index, preprocessed):
        self._ck(self._lib.vo_load_staged_pair(self._h, slot, int(index), int(bool(preprocessed))))
        return self.staged_shape

    def lookahead_depth(self):
        """Look-ahead pairs submitted and not yet waited for or dropped."""
        d = ctypes.c_int(0)
        self._ck(self._lib.vo_lookahead_depth(self._h, ctypes.byref(d)))
        return d.value

    def lookahead_drop(self, slot):
        self._ck(self._lib.vo_lookahead_drop(self._h, int(slot)))

    def sgbm_last_schedule(self):
        """SCHED_* of the latest SGBM run of this context."""
        d = ctypes.c_int(0)
        self._ck(self._lib.vo_sgbm_last_schedule(self._h, ctypes.byref(d)))
        return d.value

    def prefetch_staged_pair(self, slot, index, preprocessed):
        self._ck(self._lib.vo_prefetch_staged_pair(self._h, slot, int(index), int(bool(preprocessed))))
        return self.staged_shape

    def sgbm_compute(self, slot, shape=None):
        out = np.empty(shape, np.int16) if shape is not None else None
        self._ck(self._lib.vo_sgbm_compute(self._h, slot, _p(out)))
        return out

    def sgbm_compute_host(self, left, right):
        left, right = _c(left, np.uint8), _c(right, np.uint8)
        h, w = left.shape
        out = np.empty((h, w), np.int16)
        self._ck(self._lib.vo_sgbm_compute_host(self._h, _p(left), _p(right), w, h, _p(out)))
        return out

    def download_disparity_f32(self, slot, shape):
        out = np.empty(shape, np.float32)
        self._ck(self._lib.vo_download_disparity_f32(self._h, slot, _p(out)))
        return out

    def download_xyz(self, slot, shape):
        out = np.empty(tuple(shape) + (3,), np.float32)
        self._ck(self._lib.vo_download_xyz(self._h, slot, _p(out)))
        return out

    def download_left(self, slot, shape, right=False):
        out = np.empty(shape, np.uint8)
        f = self._lib.vo_download_right if right else self._lib.vo_download_left
        self._ck(f(self._h, slot, _p(out)))
        return out

    def cvt_bgr2gray(self, bgr):
        bgr = _c(bgr, np.uint8)
        h, w = bgr.shape[:2]
        out = np.empty((h, w), np.uint8)
        self._ck(self._lib.vo_cvt_bgr2gray(self._h, _p(bgr), w, h, _p(out)))
        return out

    def remap(self, cam, src, out_shape):
        src = _c(src, np.uint8)
        out = np.empty(out_shape, np.uint8)
        self._ck(self._lib.vo_remap(self._h, cam, _p(src), src.shape[1], src.shape[0], _p(out)))
        return out

    def reproject_to_3d(self, disp, Q):
        disp, Q = _c(disp, np.float32), _c(Q, np.float64)
        out = np.empty(disp.shape + (3,), np.float32)
        self._ck(self._lib.vo_reproject_to_3d(self._h, _p(disp), disp.shape[1], disp.shape[0], _p(Q), _p(out)))
        return out

    # ---- features
    def _kp_buffers(self, cap):
        return dict(xy=np.empty((cap, 2), np.float32), size=np.empty(cap, np.float32),
                    angle=np.empty(cap, np.float32), response=np.empty(cap, np.float32),
                    octave=np.empty(cap, np.int32), desc=np.empty((cap, 32), np.uint8))

    @staticmethod
    def _kp_args(b):
        """the six keypoint output pointers, in the order every keypoint-returning entry takes them"""
        return [_p(b[k]) for k in ("xy", "size", "angle", "response", "octave", "desc")]

    @staticmethod
    def _trim(b, n):
        return {k: v[:n] for k, v in b.items()}

    def lookahead_orb(self, nfeatures, mask_mode, min_d16, max_d16):
        """Ask the look-ahead engines to extract keypoints with these parameters behind each prefetched SGBM."""
        key = (int(nfeatures), int(mask_mode), int(min_d16), int(max_d16))
        if key != self._la_orb:
            self._ck(self._lib.vo_set_lookahead_orb(self._h, 1, *key))
            self._la_orb = key

    def lookahead_orb_off(self):
        """The look-ahead engines stop extracting keypoints behind each prefetched SGBM."""
        self._ck(self._lib.vo_set_lookahead_orb(self._h, 0, 0, 0, 0, 0))
        self._la_orb = None

    def orb_slot(self, slot, nfeatures, mask_mode, min_d16=0, max_d16=0):
        cap = self.kp_cap
        b = self._kp_buffers(cap)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_orb_detect_and_compute(self._h, slot, int(nfeatures), int(mask_mode), int(min_d16),
                                                     int(max_d16), *self._kp_args(b), cap, ctypes.byref(n)))
        return self._trim(b, n.value)

    def orb_slot_count(self, slot, nfeatures, mask_mode, min_d16=0, max_d16=0):
        """Same extraction, everything stays on the device: returns only the keypoint count."""
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_orb_detect_and_compute(self._h, slot, int(nfeatures), int(mask_mode), int(min_d16),
                                                     int(max_d16), None, None, None, None, None, None, 0, ctypes.byref(n)))
        return n.value

    def download_keypoints(self, slot):
        cap = self.kp_cap
        b = self._kp_buffers(cap)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_download_keypoints(self._h, slot, *self._kp_args(b), cap, ctypes.byref(n)))
        return self._trim(b, n.value)

    def download_keypoints_xy(self, slot):
        """Only the (n, 2) float32 positions of a slot's keypoints (the other fields stay on the device)."""
        cap = self.kp_cap
        xy = np.empty((cap, 2), np.float32)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_download_keypoints(self._h, slot, _p(xy), None, None, None, None, None, cap, ctypes.byref(n)))
        return xy[:n.value]

    def orb_host(self, img, mask, nfeatures):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("ORB input must be a 2-D uint8 image")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        h, w = img.shape
        mstride = 0
        if mask is not None:
            mask = np.asarray(mask, dtype=np.uint8)
            if mask.shape != img.shape:
                raise ValueError("mask shape differs from image shape")
            if mask.strides[1] != 1:
                mask = np.ascontiguousarray(mask)
            mstride = mask.strides[0]
        cap = self.kp_cap
        b = self._kp_buffers(cap)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_orb_detect_and_compute_host(self._h, _p(img), w, h, img.strides[0], _p(mask), mstride,
                                                          int(nfeatures), *self._kp_args(b), cap, ctypes.byref(n)))
        return self._trim(b, n.value)

    # ---- sparse stereo depth
    def sparse_stereo(self, slot, nfeatures, min_disp, max_disp, row_tol=2.0, max_hamming=75):
        """ORB on both images of the slot's pair, association along the row, sub-pixel refinement, 3-D (vo_sparse_stereo): the slot
        then holds the left keypoints that have a depth, and they carry it.  -> counts3 = [left keypoints, accepted, kept]."""
        c3 = np.zeros(3, np.int32)
        self._ck(self._lib.vo_sparse_stereo(self._h, int(slot), int(nfeatures), float(min_disp), float(max_disp), float(row_tol),
                                            int(max_hamming), _p(c3)))
        return c3

    def set_sparse_assoc(self, mutual=False, ratio=None):
        """The association tests of every sparse chain enqueued from now on (vo_set_sparse_assoc): mutual = a right keypoint
        belongs to its best left claimant only; ratio (None = off, else 0 < ratio <= 1) = the winner's distance must be below
        ratio x the runner-up's.  Remembered here: setting the state that is already in force makes no native call."""
        state = sparse_assoc_state(mutual, ratio)
        if state != self._sparse_assoc:
            self._ck(self._lib.vo_set_sparse_assoc(self._h, state[0], state[1]))
            self._sparse_assoc = state

    def download_keypoint_rdesc(self, slot):
        """-> (n, 32) uint8: the descriptor of the right keypoint each of the slot's keypoints was associated with (VoError when
        the slot's keypoints carry no depth)."""
        cap = self.kp_cap
        rdesc = np.empty((cap, 32), np.uint8)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_download_keypoint_rdesc(self._h, int(slot), _p(rdesc), cap, ctypes.byref(n)))
        return rdesc[:n.value].copy()

    def plant_keypoints(self, slot, xy, desc, xyz, rdesc=None):
        """Test-only build of the library: n keypoints (xy (n, 2), desc (n, 32), xyz (n, 3)[, rdesc (n, 32)]) straight into a slot,
        which then stands as sparse_stereo leaves it (vo_test_plant_keypoints).  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_plant_keypoints"):
            raise RuntimeError("plant_keypoints needs the test-only build of the library (libvo355_hooks.so)")
        xy, desc, xyz = _c(xy, np.float32).reshape(-1, 2), _c(desc, np.uint8).reshape(-1, 32), _c(xyz, np.float32).reshape(-1, 3)
        n = len(xy)
        if len(desc) != n or len(xyz) != n:
            raise ValueError("one descriptor and one 3-D point per keypoint")
        if rdesc is not None:
            rdesc = _c(rdesc, np.uint8).reshape(-1, 32)
            if len(rdesc) != n:
                raise ValueError("one right descriptor per keypoint")
        self._ck(self._lib.vo_test_plant_keypoints(self._h, int(slot), n, _p(xy), _p(desc), _p(xyz), _p(rdesc)))

    def plant_dense(self, slot, disp16, xy, desc):
        """Test-only build of the library: a disparity image (h, w) int16 in 1/16 px and n keypoints (xy (n, 2), desc (n, 32)) straight
        into a slot, which then stands as sgbm_compute followed by an ORB extraction leaves it (vo_test_plant_dense): the keypoints
        carry no depth.  Positions outside the crop under the ROI in force are refused.  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_plant_dense"):
            raise RuntimeError("plant_dense needs the test-only build of the library (libvo355_hooks.so)")
        disp16 = _c(disp16, np.int16)
        if disp16.ndim != 2:
            raise ValueError("disp16 is a (h, w) image")
        xy, desc = _c(xy, np.float32).reshape(-1, 2), _c(desc, np.uint8).reshape(-1, 32)
        n = len(xy)
        if len(desc) != n:
            raise ValueError("one descriptor per keypoint")
        h, w = disp16.shape
        self._ck(self._lib.vo_test_plant_dense(self._h, int(slot), w, h, _p(disp16), n, _p(xy), _p(desc)))

    def download_keypoint_depth(self, slot):
        """-> (xyz (n, 3) float32, disparity (n,) float32) of a slot whose keypoints carry depth (VoError otherwise)."""
        cap = self.kp_cap
        xyz, disp = np.empty((cap, 3), np.float32), np.empty(cap, np.float32)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_download_keypoint_depth(self._h, int(slot), _p(xyz), _p(disp), cap, ctypes.byref(n)))
        return xyz[:n.value].copy(), disp[:n.value].copy()

    def sparse_match_host(self, left, right, xy_l, oct_l, desc_l, xy_r, oct_r, desc_r, min_disp, max_disp, row_tol=2.0, max_hamming=75):
        """Association + refinement of vo_sparse_stereo on host arrays -> (match (nl,) int32, -1 = none; disparity (nl,) float32,
        NaN = rejected)."""
        left, right = _c(left, np.uint8), _c(right, np.uint8)
        if left.ndim != 2 or left.shape != right.shape:
            raise ValueError("two 2-D uint8 images of one shape")
        h, w = left.shape
        xy_l, xy_r = _c(xy_l, np.float32).reshape(-1, 2), _c(xy_r, np.float32).reshape(-1, 2)
        oct_l, oct_r = _c(oct_l, np.int32).reshape(-1), _c(oct_r, np.int32).reshape(-1)
        desc_l, desc_r = _c(desc_l, np.uint8).reshape(-1, 32), _c(desc_r, np.uint8).reshape(-1, 32)
        nl, nr = len(xy_l), len(xy_r)
        if len(oct_l) != nl or len(desc_l) != nl or len(oct_r) != nr or len(desc_r) != nr:
            raise ValueError("one octave and one descriptor per keypoint")
        match, disp = np.full(nl, -1, np.int32), np.full(nl, np.nan, np.float32)
        self._ck(self._lib.vo_sparse_match_host(self._h, _p(left), _p(right), w, h, _p(xy_l), _p(oct_l), _p(desc_l), nl, _p(xy_r), _p(oct_r),
                                                _p(desc_r), nr, float(min_disp), float(max_disp), float(row_tol), int(max_hamming),
                                                _p(match), _p(disp)))
        return match, disp

    def sparse_pair_host(self, left, right, xy_l, oct_l, desc_l, xy_r, oct_r, desc_r, Q, roi_xy, min_disp, max_disp, row_tol=2.0, max_hamming=75,
                         mutual=False, assoc_ratio=None):
        """Association, refinement AND compaction of vo_sparse_stereo on host arrays in one launch (vo_sparse_pair_host_ex) -> dict:
        match (nl,), disp (nl,) as sparse_match_host; xy, octave, desc, kp_disp, xyz, rdesc of the survivors in their order; counts3.
        mutual / assoc_ratio: the association tests as set_sparse_assoc takes them (arguments here: the context's state is not touched)."""
        aflags, aratio = sparse_assoc_state(mutual, assoc_ratio)
        left, right = _c(left, np.uint8), _c(right, np.uint8)
        if left.ndim != 2 or left.shape != right.shape:
            raise ValueError("two 2-D uint8 images of one shape")
        h, w = left.shape
        xy_l, xy_r = _c(xy_l, np.float32).reshape(-1, 2), _c(xy_r, np.float32).reshape(-1, 2)
        oct_l, oct_r = _c(oct_l, np.int32).reshape(-1), _c(oct_r, np.int32).reshape(-1)
        desc_l, desc_r = _c(desc_l, np.uint8).reshape(-1, 32), _c(desc_r, np.uint8).reshape(-1, 32)
        nl, nr = len(xy_l), len(xy_r)
        if len(oct_l) != nl or len(desc_l) != nl or len(oct_r) != nr or len(desc_r) != nr:
            raise ValueError("one octave and one descriptor per keypoint")
        Q = _c(Q, np.float64).reshape(16)
        match, disp = np.full(nl, -1, np.int32), np.full(nl, np.nan, np.float32)
        xy, octave, desc = np.zeros((nl, 2), np.float32), np.zeros(nl, np.int32), np.zeros((nl, 32), np.uint8)
        kp_disp, xyz, c3 = np.zeros(nl, np.float32), np.zeros((nl, 3), np.float32), np.zeros(3, np.int32)
        rdesc = np.zeros((nl, 32), np.uint8)
        self._ck(self._lib.vo_sparse_pair_host_ex(self._h, _p(left), _p(right), w, h, _p(xy_l), _p(oct_l), _p(desc_l), nl, _p(xy_r), _p(oct_r),
                                                  _p(desc_r), nr, float(min_disp), float(max_disp), float(row_tol), int(max_hamming), aflags,
                                                  aratio, _p(Q), int(roi_xy[0]), int(roi_xy[1]), _p(match), _p(disp), _p(xy), _p(octave),
                                                  _p(desc), _p(kp_disp), _p(xyz), _p(rdesc), _p(c3)))
        n = int(c3[2])
        return dict(match=match, disp=disp, xy=xy[:n], octave=octave[:n], desc=desc[:n], kp_disp=kp_disp[:n], xyz=xyz[:n], rdesc=rdesc[:n],
                    counts3=c3)

    # ---- matching / 3-D / pose
    def bf_knn2(self, q, t):
        q, t = _c(q, np.uint8).reshape(-1, 32), _c(t, np.uint8).reshape(-1, 32)
        idx = np.empty((len(q), 2), np.int32)
        dist = np.empty((len(q), 2), np.int32)
        self._ck(self._lib.vo_bf_knn2_hamming(self._h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)))
        return idx, dist

    def set_match_loop(self, max_hamming):
        """the threshold of the loop check (VO_MATCH_LOOP) for the steps enqueued from now on; remembered: the value in force makes no native call"""
        n = loop_threshold(max_hamming)
        if n is None:
            raise ValueError("loop is an int in 0 .. 256 (clear_match_loop takes it away)")
        if n != self._loop:
            self._ck(self._lib.vo_set_match_loop(self._h, n))
            self._loop = n

    def clear_match_loop(self):
        self._ck(self._lib.vo_clear_match_loop(self._h))
        self._loop = None

    def _mflags(self, cross_check, window, loop=None):
        """match_flags of the _ex entries; a window / a loop threshold goes into the context first (only when it differs from the
        last one set)"""
        f = _flags(cross_check)
        if loop is not None:
            self.set_match_loop(loop)
            f |= VO_MATCH_LOOP
        w = window_radii(window)
        if w is not None:
            if w != self._window:
                self._ck(self._lib.vo_set_match_window(self._h, w[0], w[1]))
                self._window = w
            f |= VO_MATCH_WINDOW
        return f

    def bf_knn2_window(self, q, t, xy_q, xy_t, window, cross_check=False):
        """kNN-2 among the trains inside the window (rx, ry) around each query's position: |xq - xt| <= rx and |yq - yt| <= ry in
        float32, a NaN coordinate in no window -> (idx, dist), {-1, INT32_MAX} where a query has fewer than two candidates; with
        cross_check (idx, dist, mutual, t_best) as bf_knn2_mutual, mutual within the window."""
        w = window_radii(window)
        if w is None:
            raise ValueError("bf_knn2_window needs a window")
        q, t = _c(q, np.uint8).reshape(-1, 32), _c(t, np.uint8).reshape(-1, 32)
        xy_q, xy_t = _c(xy_q, np.float32).reshape(-1, 2), _c(xy_t, np.float32).reshape(-1, 2)
        if len(xy_q) != len(q) or len(xy_t) != len(t):
            raise ValueError("one position per descriptor")
        idx = np.empty((len(q), 2), np.int32)
        dist = np.empty((len(q), 2), np.int32)
        mutual = np.empty(len(q), np.uint8) if cross_check else None
        t_best = np.empty((len(t), 2), np.int32) if cross_check else None
        self._ck(self._lib.vo_bf_knn2_hamming_window(self._h, _p(q), len(q), _p(t), len(t), _p(xy_q), _p(xy_t), w[0], w[1],
                                                     VO_MATCH_WINDOW | _flags(cross_check), _p(idx), _p(dist), _p(mutual), _p(t_best)))
        return (idx, dist, mutual, t_best) if cross_check else (idx, dist)

    def bf_knn2_mutual(self, q, t):
        """bf_knn2 plus the cross-check of the same launch -> (idx, dist, mutual, t_best): mutual[i] = 1 when the nearest train of
        query i has query i as ITS nearest query (ties -> lower index both ways); t_best (nt x 2) = that nearest query of every
        train descriptor and its distance ({-1, INT32_MAX} when there is no query)."""
        q, t = _c(q, np.uint8).reshape(-1, 32), _c(t, np.uint8).reshape(-1, 32)
        idx = np.empty((len(q), 2), np.int32)
        dist = np.empty((len(q), 2), np.int32)
        mutual = np.empty(len(q), np.uint8)
        t_best = np.empty((len(t), 2), np.int32)
        self._ck(self._lib.vo_bf_knn2_hamming_mutual(self._h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist), _p(mutual), _p(t_best)))
        return idx, dist, mutual, t_best

    def ratio_filter(self, idx, dist, ratio):
        idx, dist = _c(idx, np.int32), _c(dist, np.int32)
        qo, to = np.empty(len(idx), np.int32), np.empty(len(idx), np.int32)
        m = ctypes.c_int(0)
        rc = self._lib.vo_ratio_filter(_p(idx), _p(dist), len(idx), float(ratio), _p(qo), _p(to), ctypes.byref(m))
        if rc != 0:
            raise IndexError("list index out of range")  # what m[1] raises in the reference
        return qo[:m.value], to[:m.value]

    def points3d_at(self, slot, xy):
        xy = _c(xy, np.float32).reshape(-1, 2)
        out = np.empty((len(xy), 3), np.float32)
        st = np.empty(len(xy), np.uint8)
        self._ck(self._lib.vo_points3d_at(self._h, slot, _p(xy), len(xy), _p(out), _p(st)))
        return out, st

    def bilinear_at(self, img3d, xy):
        img3d, xy = _c(img3d, np.float32), _c(xy, np.float32).reshape(-1, 2)
        h, w = img3d.shape[:2]
        out = np.empty((len(xy), 3), np.float32)
        st = np.empty(len(xy), np.uint8)
        self._ck(self._lib.vo_bilinear_at(self._h, _p(img3d), w, h, _p(xy), len(xy), _p(out), _p(st)))
        return out, st

    @staticmethod
    def klt_params(win=21, levels=4, iters=30, eps=0.01, min_eig=1e-4, fb=1.0):
        """the parameters of the Lucas-Kanade entries (include/vo355.h) as their C arguments; ValueError for a value the
        library would refuse"""
        def _int(v, lo, hi):
            return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and lo <= v <= hi
        if not _int(win, 5, 31) or win % 2 == 0:
            raise ValueError("win must be an odd int in 5 .. 31, not %r" % (win,))
        if not _int(levels, 1, 6):
            raise ValueError("levels must be an int in 1 .. 6, not %r" % (levels,))
        if not _int(iters, 1, 100):
            raise ValueError("iters must be an int in 1 .. 100, not %r" % (iters,))
        for name, v in (("eps", eps), ("min_eig", min_eig), ("fb", fb)):
            if (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0):
                raise ValueError("%s must be a finite number >= 0, not %r" % (name, v))
        return int(win), int(levels), int(iters), float(eps), float(min_eig), float(fb)

    def klt_track_host(self, a, b, xy, **kw):
        """Pyramidal Lucas-Kanade with a forward-backward check (vo_klt_track_host): the points xy (n, 2; full-image pixels) of image a
        tracked into image b -> (xy_out (n, 2) float32, status (n,) uint8: 0 tracked | 1 eigenvalue | 2 left the image | 4 non-finite
        | 8 forward-backward, iters (n,) int32).  Keywords: win, levels, iters, eps, min_eig, fb."""
        prm = self.klt_params(**kw)
        (a, ch_a), (b, ch_b) = _image(a), _image(b)
        if ch_a != 1 or ch_b != 1 or a.shape != b.shape:
            raise ValueError("klt_track_host takes two grey images of one shape")
        xy = _c(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        out, st, it = np.empty((n, 2), np.float32), np.empty(n, np.uint8), np.empty(n, np.int32)
        self._ck(self._lib.vo_klt_track_host(self._h, _p(a), _p(b), a.shape[1], a.shape[0], _p(xy), n, *prm, _p(out), _p(st), _p(it)))
        return out, st, it

    def klt_track(self, slot_a, slot_b, **kw):
        """vo_klt_track: slot_a's keypoints (ROI-cropped pixels) tracked from slot_a's rectified left image into slot_b's
        -> (xy_out, status, iters) as klt_track_host, in keypoint order and ROI-cropped pixels"""
        prm = self.klt_params(**kw)
        cap = self.kp_cap
        out, st, it = np.empty((cap, 2), np.float32), np.empty(cap, np.uint8), np.empty(cap, np.int32)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_klt_track(self._h, slot_a, slot_b, *prm, _p(out), _p(st), _p(it), cap, ctypes.byref(n)))
        n = n.value
        return out[:n].copy(), st[:n].copy(), it[:n].copy()

    # ---- the Lucas-Kanade PnP pair step (vo_klt_pnp_pair)
    def _klt_pnp_front(self, slot_a, slot_b, K4, iters, thr, seed, refine, lo_rounds, klt):
        """the input arguments the three entries share, checked as the library checks them"""
        klt = dict(klt)
        if "klt_iters" in klt:                   # (`iters` is the RANSAC's here: the tracker's iteration limit travels as klt_iters)
            klt["iters"] = klt.pop("klt_iters")
        prm = self.klt_params(**klt)
        lo_rounds = self.lo_rounds_arg(lo_rounds, refine)
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        return [self._h, int(slot_a), int(slot_b), *prm, _p(K4), int(iters), float(thr), int(seed) & 0xFFFFFFFF, int(refine), lo_rounds], K4

    def _klt_pnp_out(self, want_arrays):
        head = [np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(12, np.float64), np.zeros(12, np.float64), np.zeros(2, np.int32),
                np.zeros(2, np.int32)]
        arrays = [None, None, None]
        if want_arrays:
            arrays = self.__dict__.get("_klt_pnp_arrays")
            if arrays is None or len(arrays[0]) != self.kp_cap:
                arrays = self._klt_pnp_arrays = [np.empty(self.kp_cap, np.uint8), np.empty(self.kp_cap, np.int32), np.empty((self.kp_cap, 2), np.float32)]
        return head, arrays

    @staticmethod
    def _klt_pnp_result(head, arrays):
        out = Context._pnp_result(head[:5], [arrays[0], arrays[1], arrays[1]])
        out.pop("t", None)
        out.update(lo_rounds=int(head[5][0]), lo_support=int(head[5][1]))
        if arrays[0] is not None:
            out["xy"] = arrays[2][:out["n"]].copy()
        return out

    def klt_pnp_pair(self, slot_a, slot_b, K4, iters=256, thr=1.5, seed=4321, refine=0, lo_rounds=0, want_arrays=False, **klt):
        """slot_a's keypoints tracked into slot_b (Lucas-Kanade: keywords win, levels, klt_iters, eps, min_eig, fb -- klt_track's,
        its iteration limit as klt_iters), the 3-D points of the kept tracks in slot_a, P3P RANSAC (+ refit, + LO rounds), all on the device with one
        synchronisation (vo_klt_pnp_pair).  -> the dict of pnp_pair (matches = the tracks with status 0; lo_rounds / lo_support as
        pnp_pair_lo) [, mask, q, xy of length n: xy = the tracked positions, ROI-cropped pixels]."""
        front, _keep = self._klt_pnp_front(slot_a, slot_b, K4, iters, thr, seed, refine, lo_rounds, klt)
        head, arrays = self._klt_pnp_out(want_arrays)
        self._ck(self._lib.vo_klt_pnp_pair(*front, *[_p(a) for a in head + arrays], self.kp_cap))
        return self._klt_pnp_result(head, arrays)

    def klt_pnp_pair_begin(self, slot_a, slot_b, K4, iters=256, thr=1.5, seed=4321, refine=0, lo_rounds=0, want_arrays=False, **klt):
        """klt_pnp_pair in two halves -> a ticket for klt_pnp_pair_end (a pose ticket: VO_NUM_POSE_ASYNC bounds all kinds together)."""
        front, _keep = self._klt_pnp_front(slot_a, slot_b, K4, iters, thr, seed, refine, lo_rounds, klt)
        t = ctypes.c_int(-1)
        self._ck(self._lib.vo_klt_pnp_pair_begin(*front, int(bool(want_arrays)), ctypes.byref(t)))
        return t.value

    def klt_pnp_pair_end(self, ticket, want_arrays=False):
        head, arrays = self._klt_pnp_out(want_arrays)
        self._ck(self._lib.vo_klt_pnp_pair_end(self._h, int(ticket), *[_p(a) for a in head + arrays], self.kp_cap))
        return self._klt_pnp_result(head, arrays)

    # ---- dense direct alignment (vo_direct_align)
    @staticmethod
    def direct_params(levels=3, iters=8, max_points=16384, grad_min=8, huber=10.0, dmin=4.0, dmax=100.0, z_min=0.1, min_pixels=64):
        """the parameters of direct_align as the library takes them, checked as the library checks them (ValueError)"""
        def _int(v, lo, hi):
            return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and lo <= v <= hi

        def _num(v):
            return not isinstance(v, (bool, np.bool_, str, bytes)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if not _int(levels, 1, DIRECT_MAX_LEVELS):
            raise ValueError("levels is an int in 1 .. %d, not %r" % (DIRECT_MAX_LEVELS, levels))
        if not _int(iters, 1, 20):
            raise ValueError("iters is an int in 1 .. 20, not %r" % (iters,))
        if not _int(max_points, 1, 2 ** 31 - 1):
            raise ValueError("max_points is an int >= 1, not %r" % (max_points,))
        if not _int(grad_min, 0, 255):
            raise ValueError("grad_min is an int in 0 .. 255, not %r" % (grad_min,))
        if not _int(min_pixels, 6, 2 ** 31 - 1):
            raise ValueError("min_pixels is an int >= 6, not %r" % (min_pixels,))
        if not (_num(huber) and huber > 0):
            raise ValueError("huber is a finite number > 0, not %r" % (huber,))
        if not (_num(dmin) and _num(dmax) and 0 < dmin <= dmax):
            raise ValueError("dmin and dmax are finite numbers with 0 < dmin <= dmax, not %r, %r" % (dmin, dmax))
        if not (_num(z_min) and z_min >= 0):
            raise ValueError("z_min is a finite number >= 0, not %r" % (z_min,))
        return (int(levels), int(iters), int(max_points), int(grad_min), float(huber), float(dmin), float(dmax), float(z_min), int(min_pixels))

    def direct_align(self, slot_a, slot_b, K4, Rt0=None, levels=3, iters=8, max_points=16384, grad_min=8, huber=10.0, dmin=4.0, dmax=100.0,
                     z_min=0.1, min_pixels=64, affine=False):
        """Photometric refinement of the a -> b motion on slot_a's dense disparity (vo_direct_align, include/vo355.h): slot_a's
        rectified left image and disparity against slot_b's rectified left image, from Rt0 (3 x 4 or 4 x 4, X' = R X + t; None: the
        identity), one launch and one synchronisation.  -> dict: status (0 all iterations ran | 2 starved | -1 numeric), iters_done,
        per level s / selected / n_first / n_last / wr2_first / wr2_last, Rt (3, 4), information (6, 6: sum w j j^T of the last
        completed linearisation, rotation then translation), g (6), count, wr2, sums (the 27 raw sums).
        affine=True (vo_direct_align_ab; iters 3 .. 20): a gain and an offset of slot_b's brightness are estimated beside the pose,
        from the third iteration of every level on.  The dict then adds gain, offset, unknowns (6 or 8: the size of the last completed
        linearisation), information_full (8, 8: pose, gain, offset; zero outside the 6 x 6 block when unknowns == 6); sums are the 44
        raw sums, g has 8 entries, and information is the pose information MARGINALISED over the brightness, H_pp - H_pb H_bb^-1 H_bp
        (the plain 6 x 6 when unknowns == 6)."""
        if not isinstance(affine, (bool, np.bool_)):
            raise ValueError("affine must be True or False")
        entry = "vo_direct_align_ab" if affine else "vo_direct_align"
        if not hasattr(self._lib, entry):
            raise RuntimeError("this build of the library has no dense direct alignment (%s)" % entry)
        prm = self.direct_params(levels, iters, max_points, grad_min, huber, dmin, dmax, z_min, min_pixels)
        if affine and prm[1] < 3:
            raise ValueError("affine=True needs iters in 3 .. 20 (the first two iterations of a level hold the brightness), not %r" % (iters,))
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        Rt = np.eye(4)[:3] if Rt0 is None else np.asarray(Rt0, np.float64)
        if Rt.shape == (4, 4):
            Rt = Rt[:3]
        Rt = _c(Rt.reshape(12), np.float64)
        rec = DirectAbRec() if affine else DirectRec()
        self._ck(getattr(self._lib, entry)(self._h, int(slot_a), int(slot_b), _p(K4), _p(Rt), *prm, ctypes.byref(rec)))
        return rec.as_dict()

    # ---- patch alignment (vo_direct_align_kp)
    @staticmethod
    def direct_kp_params(levels=3, iters=4, patch=5, grad_min=8, huber=10.0, z_min=0.1, min_pixels=64):
        """the parameters of direct_align_kp as the library takes them, checked as the library checks them (ValueError)"""
        if isinstance(patch, (bool, np.bool_)) or not isinstance(patch, (int, np.integer)) or patch not in (3, 5, 7):
            raise ValueError("patch is 3, 5 or 7, not %r" % (patch,))
        p = Context.direct_params(levels=levels, iters=iters, grad_min=grad_min, huber=huber, z_min=z_min, min_pixels=min_pixels)
        return (p[0], p[1], int(patch), p[3], p[4], p[7], p[8])

    def direct_align_kp(self, slot_a, slot_b, K4, Rt0=None, levels=3, iters=4, patch=5, grad_min=8, huber=10.0, z_min=0.1, min_pixels=64):
        """Photometric refinement of the a -> b motion on slot_a's depth-carrying keypoints (vo_direct_align_kp, include/vo355.h): a
        patch x patch pixel patch around every keypoint of slot_a (a sparse slot), each pixel at its keypoint's depth, against slot_b's
        rectified left image, from Rt0 (3 x 4 or 4 x 4; None: the identity); one launch and one synchronisation.  -> the dict of
        direct_align, with `keypoints` (per level: the keypoints whose patch lies in the level's rectangle) in the place of `s`, and
        `patch`."""
        if not hasattr(self._lib, "vo_direct_align_kp"):
            raise RuntimeError("this build of the library has no patch alignment (vo_direct_align_kp)")
        prm = self.direct_kp_params(levels, iters, patch, grad_min, huber, z_min, min_pixels)
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        Rt = np.eye(4)[:3] if Rt0 is None else np.asarray(Rt0, np.float64)
        if Rt.shape == (4, 4):
            Rt = Rt[:3]
        Rt = _c(Rt.reshape(12), np.float64)
        rec = DirectRec()
        self._ck(self._lib.vo_direct_align_kp(self._h, int(slot_a), int(slot_b), _p(K4), _p(Rt), *prm, ctypes.byref(rec)))
        d = rec.as_dict()
        d["keypoints"] = d.pop("s")
        d["patch"] = int(rec.pad)
        return d

    def plant_dense_pair(self, slot, left, disp16, xy, desc=None):
        """Test-only build of the library: plant_dense, and the (h, w) uint8 image `left` as the slot's rectified pair
        (vo_test_plant_dense_pair): a dense slot that can be tracked from.  desc defaults to zeros.  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_plant_dense_pair"):
            raise RuntimeError("plant_dense_pair needs the test-only build of the library (libvo355_hooks.so)")
        left, disp16 = _c(left, np.uint8), _c(disp16, np.int16)
        if left.ndim != 2 or left.shape != disp16.shape:
            raise ValueError("left and disp16 are (h, w) images of one shape")
        xy = _c(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        desc = np.zeros((n, 32), np.uint8) if desc is None else _c(desc, np.uint8).reshape(-1, 32)
        if len(desc) != n:
            raise ValueError("one descriptor per keypoint")
        h, w = disp16.shape
        self._ck(self._lib.vo_test_plant_dense_pair(self._h, int(slot), w, h, _p(left), _p(disp16), n, _p(xy), _p(desc)))

    def klt_level(self, which, level, w_l, h_l):
        """Test-only build of the library: level `level` (w_l x h_l) of the pyramid of image `which` (0 = a, 1 = b) as the last
        klt_track_host left it (vo_test_klt_level) -> (h_l, w_l) uint8.  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_klt_level"):
            raise RuntimeError("klt_level needs the test-only build of the library (libvo355_hooks.so)")
        out = np.empty((max(int(h_l), 0), max(int(w_l), 0)), np.uint8)
        self._ck(self._lib.vo_test_klt_level(self._h, int(which), int(level), int(w_l), int(h_l), _p(out)))
        return out

    def point_clouds(self, slot_a, slot_b, ratio, cross_check=False, window=None, loop=None):
        """loop (None | 0 .. 256): the loop check on two slots whose keypoints carry depth (VO_MATCH_LOOP)"""
        cap = self.kp_cap
        q, t = np.empty(cap, np.int32), np.empty(cap, np.int32)
        pa, pb = np.empty((cap, 3), np.float32), np.empty((cap, 3), np.float32)
        sa, sb = np.empty(cap, np.uint8), np.empty(cap, np.uint8)
        m = ctypes.c_int(0)
        self._ck(self._lib.vo_point_clouds_ex(self._h, slot_a, slot_b, float(ratio), self._mflags(cross_check, window, loop), _p(q), _p(t), _p(pa), _p(pb),
                                              _p(sa), _p(sb), cap, ctypes.byref(m)))
        m = m.value
        return q[:m], t[:m], pa[:m], pb[:m], sa[:m], sb[:m]

    @staticmethod
    def _pose_out():
        """(counts[M, n1, n2, flags], rc[first, final], T1 3x4, T2 3x4) as the pose entries expect them on entry"""
        return np.zeros(4, np.int32), np.ones(2, np.int32), np.full((3, 4), np.nan), np.full((3, 4), np.nan)

    def pose_pair(self, slot_a, slot_b, ratio, min_matches, rigidity_thr, outlier_thr, cross_check=False, window=None, loop=None):
        """Fused match + ratio + 3-D lookup + clique filter + outlier pass + Umeyama for two slots.
        Returns (counts[M, n1, n2, flags], rc[first, final], T1 3x4, T2 3x4)."""
        out = self._pose_out()
        self._ck(self._lib.vo_pose_pair_ex(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), int(min_matches),
                                           float(rigidity_thr), float(outlier_thr), *[_p(a) for a in out]))
        return out

    def pose_pair_begin(self, slot_a, slot_b, ratio, min_matches, rigidity_thr, outlier_thr, cross_check=False, window=None, loop=None):
        t = ctypes.c_int(-1)
        self._ck(self._lib.vo_pose_pair_begin_ex(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), int(min_matches),
                                                 float(rigidity_thr), float(outlier_thr), ctypes.byref(t)))
        return t.value

    def pose_pair_end(self, ticket):
        out = self._pose_out()
        self._ck(self._lib.vo_pose_pair_end(self._h, int(ticket), *[_p(a) for a in out]))
        return out

    def ransac_essential(self, pts1, pts2, K4, iters=5000, thr=1.0, seed=4321, want_counts=False, solver=8):
        if solver not in (5, 8):
            raise ValueError("solver is 5 (five-point) or 8 (eight-point)")
        pts1, pts2 = _c(pts1, np.float32).reshape(-1, 2), _c(pts2, np.float32).reshape(-1, 2)
        if len(pts1) != len(pts2):
            raise ValueError("point sets differ in length")
        K4 = _c(K4, np.float64)
        n = len(pts1)
        E = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        counts = np.zeros(iters, np.int32) if want_counts else None
        best = np.zeros(2, np.int32)
        fn = self._lib.vo_ransac_essential5 if solver == 5 else self._lib.vo_ransac_essential
        self._ck(fn(self._h, _p(pts1), _p(pts2), n, _p(K4), int(iters), float(thr), int(seed), _p(E), _p(mask), _p(counts), _p(best)))
        return dict(E=E.reshape(3, 3), mask=mask, counts=counts, best_iter=int(best[0]), best_count=int(best[1]))

    def upload_mono(self, slot, img):
        """One image into a slot (monocular front end)."""
        img, ch = _image(img)      # HxWx4 / HxWx2 are refused before native code would read w*h*3 bytes from them
        h, w = img.shape[:2]
        self._ck(self._lib.vo_upload_mono(self._h, slot, _p(img), w, h, ch))
        return w, h

    def prefetch_staged_mono(self, slot, index, nfeatures):
        self._ck(self._lib.vo_prefetch_staged_mono(self._h, int(slot), int(index), int(nfeatures)))

    @staticmethod
    def _mono_result(E, c3, **arrays):
        """header of a monocular step (+ its per-match arrays cut to the M matches, xy_b whole) -> the dict mono_pair returns"""
        out = {"E": E.reshape(3, 3), "matches": int(c3[0]), "best_iter": int(c3[1]), "best_count": int(c3[2])}
        out.update((k, (v if k == "xy_b" else v[:int(c3[0])]).copy()) for k, v in arrays.items())
        return out

    def mono_pair(self, slot_a, slot_b, ratio, K4, iters=5000, thr=1.0, seed=4321, want_matches=False, solver=8, cross_check=False, window=None):
        """kNN-2 + ratio + essential-matrix RANSAC between two slots' keypoints, all on the device, one sync.
        -> dict(E 3x3, matches M, best_iter, best_count[, mask, q, t of length M])."""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        E = np.zeros(9, np.float64)
        c3 = np.zeros(3, np.int32)
        cap = self.kp_cap
        arrays = dict(mask=np.zeros(cap, np.uint8), q=np.zeros(cap, np.int32), t=np.zeros(cap, np.int32)) if want_matches else {}
        self._ck(self._lib.vo_mono_pair_ex(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window), _p(K4), int(iters), float(thr),
                                           int(seed) & 0xFFFFFFFF, int(solver), _p(E), _p(c3), _p(arrays.get("mask")), _p(arrays.get("q")),
                                           _p(arrays.get("t")), cap))
        return self._mono_result(E, c3, **arrays)

    def slot_ready(self, slot):
        r = ctypes.c_int(0)
        self._ck(self._lib.vo_slot_ready(self._h, int(slot), ctypes.byref(r)))
        return bool(r.value)

    def mono_pair_begin(self, slot_a, slot_b, ratio, K4, iters=5000, thr=1.0, seed=4321, want_matches=False, solver=8, cross_check=False, window=None):
        """mono_pair in two halves (several pairs in flight): -> ticket for mono_pair_end."""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        t = ctypes.c_int(-1)
        self._ck(self._lib.vo_mono_pair_begin_ex(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window), _p(K4), int(iters), float(thr),
                                              int(seed) & 0xFFFFFFFF, int(solver), int(bool(want_matches)), ctypes.byref(t)))
        return t.value

    def mono_pair_end(self, ticket, want_matches=False):
        """-> the dict mono_pair returns (+ "xy_b": keypoint positions of the second slot, when want_matches)."""
        E = np.zeros(9, np.float64)
        c3 = np.zeros(3, np.int32)
        cap = self.kp_cap
        arrays = {}
        if want_matches:
            # one set of output arrays per context, reused call after call (what is handed out are copies)
            arrays = self.__dict__.get("_mono_out")
            if arrays is None or len(arrays["mask"]) != cap:
                arrays = self._mono_out = dict(mask=np.empty(cap, np.uint8), q=np.empty(cap, np.int32), t=np.empty(cap, np.int32),
                                               xy_b=np.empty((cap, 2), np.float32))
        self._ck(self._lib.vo_mono_pair_end(self._h, int(ticket), _p(E), _p(c3), _p(arrays.get("mask")), _p(arrays.get("q")), _p(arrays.get("t")),
                                            _p(arrays.get("xy_b")), cap))
        return self._mono_result(E, c3, **arrays)

    def recover_pose(self, E, pts1, pts2, K4, mask=None, q_idx=None, t_idx=None, na=None, nb=None, depth_a=None, min_parallax_sin2=0.0,
                     want_depths=True):
        """E + pixel correspondences -> (R, unit t), cheirality votes over every inlier, the inliers' depths and the ratio of this
        pair's baseline to the previous one's (vo_recover_pose).  -> the record as a dict (MonoPose.as_dict) + depth_b, z1, z2."""
        E = _c(np.asarray(E, np.float64).reshape(9), np.float64)
        pts1, pts2 = _c(pts1, np.float32).reshape(-1, 2), _c(pts2, np.float32).reshape(-1, 2)
        n = len(pts1)
        if len(pts2) != n:
            raise ValueError("point sets differ in length")
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        if mask is not None:
            mask = _c(mask, np.uint8).reshape(-1)
            if len(mask) != n:
                raise ValueError("mask length differs from the point sets'")
        if (q_idx is None) != (t_idx is None):
            raise ValueError("q_idx and t_idx come together")
        if q_idx is not None:
            q_idx, t_idx = _c(q_idx, np.int32).reshape(-1), _c(t_idx, np.int32).reshape(-1)
            if len(q_idx) != n or len(t_idx) != n or na is None or nb is None:
                raise ValueError("q_idx / t_idx need one entry per correspondence, and na, nb")
        else:
            na = nb = n
        if depth_a is not None:
            depth_a = _c(depth_a, np.float64).reshape(-1)
            if len(depth_a) != int(na):
                raise ValueError("depth_a needs na entries")
        rec = MonoPose()
        depth_b = np.zeros(max(int(nb), 0), np.float64) if want_depths else None
        z1 = np.zeros(n, np.float64) if want_depths else None
        z2 = np.zeros(n, np.float64) if want_depths else None
        self._ck(self._lib.vo_recover_pose(self._h, _p(E), _p(pts1), _p(pts2), _p(mask), n, _p(K4), _p(q_idx), _p(t_idx), int(na), int(nb),
                                           _p(depth_a), float(min_parallax_sin2), ctypes.byref(rec), _p(depth_b), _p(z1), _p(z2)))
        out = rec.as_dict()
        out.update(depth_b=depth_b, z1=z1, z2=z2)
        return out

    def mono_pose_pair(self, slot_a, slot_b, ratio, K4, iters=5000, thr=1.0, seed=4321, solver=8, cross_check=False, prev_serial=0,
                       min_parallax_sin2=0.0, window=None):
        """mono_pair with the pose recovered on the device (vo_mono_pose_pair): -> the record as a dict (MonoPose.as_dict); the
        depths stay in slot_b under the record's serial."""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        rec = MonoPose()
        self._ck(self._lib.vo_mono_pose_pair(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window), _p(K4), int(iters), float(thr),
                                             int(seed) & 0xFFFFFFFF, int(solver), int(prev_serial), float(min_parallax_sin2), ctypes.byref(rec)))
        return rec.as_dict()

    def mono_pose_pair_begin(self, slot_a, slot_b, ratio, K4, iters=5000, thr=1.0, seed=4321, solver=8, cross_check=False, prev_serial=0,
                             min_parallax_sin2=0.0, window=None):
        """mono_pose_pair in two halves: -> (ticket for mono_pose_pair_end, the step's serial)."""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        t, serial = ctypes.c_int(-1), ctypes.c_uint32(0)
        self._ck(self._lib.vo_mono_pose_pair_begin(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window), _p(K4), int(iters),
                                                   float(thr), int(seed) & 0xFFFFFFFF, int(solver), int(prev_serial), float(min_parallax_sin2),
                                                   ctypes.byref(t), ctypes.byref(serial)))
        return t.value, serial.value

    def mono_pose_pair_end(self, ticket):
        rec = MonoPose()
        self._ck(self._lib.vo_mono_pose_pair_end(self._h, int(ticket), ctypes.byref(rec)))
        return rec.as_dict()

    def download_mono_depth(self, slot):
        """-> (depth of each keypoint of the slot in units of the baseline of the step that wrote them, that step's serial); serial
        0: the slot holds none (zeros)."""
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_slot_num_keypoints(self._h, int(slot), ctypes.byref(n)))
        out = np.zeros(n.value, np.float64)
        serial = ctypes.c_uint32(0)
        self._ck(self._lib.vo_download_mono_depth(self._h, int(slot), _p(out), ctypes.byref(serial)))
        return out, serial.value

    def ransac_pnp(self, pts3d, pts2d, K4, iters=5000, thr=2.0, seed=4321, want_counts=False):
        pts3d, pts2d = _c(pts3d, np.float32).reshape(-1, 3), _c(pts2d, np.float32).reshape(-1, 2)
        if len(pts3d) != len(pts2d):
            raise ValueError("point sets differ in length")
        K4 = _c(K4, np.float64)
        n = len(pts3d)
        Rt = np.zeros(12, np.float64)
        mask = np.zeros(n, np.uint8)
        counts = np.zeros(iters, np.int32) if want_counts else None
        best = np.zeros(2, np.int32)
        self._ck(self._lib.vo_ransac_pnp(self._h, _p(pts3d), _p(pts2d), n, _p(K4), int(iters), float(thr), int(seed),
                                         _p(Rt), _p(mask), _p(counts), _p(best)))
        return dict(Rt=Rt.reshape(3, 4), mask=mask, counts=counts, best_iter=int(best[0]), best_count=int(best[1]))

    def _pnp_out(self, want_matches):
        """the output arrays of the PnP pair entries, in the order they take them (mask / q / t: one set per context, reused)"""
        head = [np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(12, np.float64), np.zeros(12, np.float64), np.zeros(2, np.int32)]
        arrays = [None, None, None]
        if want_matches:
            arrays = self.__dict__.get("_pnp_arrays")
            if arrays is None or len(arrays[0]) != self.kp_cap:
                arrays = self._pnp_arrays = [np.empty(self.kp_cap, np.uint8), np.empty(self.kp_cap, np.int32), np.empty(self.kp_cap, np.int32)]
        return head, arrays

    @staticmethod
    def _pnp_result(head, arrays):
        c4, fl, Rt, Rtr, r2 = head
        n = int(c4[1])
        out = dict(matches=int(c4[0]), n=n, best_iter=int(c4[2]), best_count=int(c4[3]), flags=int(fl[0]), Rt=Rt.reshape(3, 4),
                   Rt_refined=Rtr.reshape(3, 4), refine_status=int(r2[0]), refine_steps=int(r2[1]))
        if arrays[0] is not None:
            out.update(mask=arrays[0][:n].copy(), q=arrays[1][:n].copy(), t=arrays[2][:n].copy())
        return out

    def pnp_pair(self, slot_a, slot_b, ratio, K4, iters=256, thr=1.5, seed=4321, refine=0, want_matches=False, cross_check=False):
        """kNN-2 + ratio (+ cross-check) + 3-D lookup in slot_a + P3P RANSAC (+ `refine` Gauss-Newton steps on the winner's inliers)
        for two slots, all on the device, one synchronisation (vo_pnp_pair).  -> dict(matches M, n usable correspondences,
        best_iter, best_count, flags, Rt 3x4, Rt_refined 3x4 (valid when refine_status == 0), refine_status, refine_steps
        [, mask, q, t of length n])."""
        return self.pnp_pair_window(slot_a, slot_b, ratio, K4, None, iters, thr, seed, refine, want_matches, cross_check)

    def pnp_pair_window(self, slot_a, slot_b, ratio, K4, window, iters=256, thr=1.5, seed=4321, refine=0, want_matches=False, cross_check=False,
                        loop=None):
        """pnp_pair with the kNN-2 inside the match window (None | (rx, ry), see bf_knn2_window) and / or the loop check (loop:
        None | 0 .. 256).  A method of its own: the signature of pnp_pair is pinned by the callers that bind against it."""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        head, arrays = self._pnp_out(want_matches)
        self._ck(self._lib.vo_pnp_pair(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), _p(K4), int(iters), float(thr),
                                       int(seed) & 0xFFFFFFFF, int(refine), *[_p(a) for a in head + arrays], self.kp_cap))
        return self._pnp_result(head, arrays)

    def pnp_pair_begin(self, slot_a, slot_b, ratio, K4, iters=256, thr=1.5, seed=4321, refine=0, want_matches=False, cross_check=False):
        """pnp_pair in two halves -> a ticket for pnp_pair_end (a pose ticket: VO_NUM_POSE_ASYNC bounds both kinds together)."""
        return self.pnp_pair_begin_window(slot_a, slot_b, ratio, K4, None, iters, thr, seed, refine, want_matches, cross_check)

    def pnp_pair_begin_window(self, slot_a, slot_b, ratio, K4, window, iters=256, thr=1.5, seed=4321, refine=0, want_matches=False,
                              cross_check=False, loop=None):
        """pnp_pair_window in two halves -> a ticket for pnp_pair_end"""
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        t = ctypes.c_int(-1)
        self._ck(self._lib.vo_pnp_pair_begin(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), _p(K4), int(iters), float(thr),
                                             int(seed) & 0xFFFFFFFF, int(refine), int(bool(want_matches)), ctypes.byref(t)))
        return t.value

    def pnp_pair_end(self, ticket, want_matches=False):
        head, arrays = self._pnp_out(want_matches)
        self._ck(self._lib.vo_pnp_pair_end(self._h, int(ticket), *[_p(a) for a in head + arrays], self.kp_cap))
        return self._pnp_result(head, arrays)

    # ---- the PnP step with local-optimisation rounds (vo_pnp_pair_lo; new methods: the signatures above are pinned)
    @staticmethod
    def lo_rounds_arg(lo_rounds, refine):
        """int 0 .. 8, and a value above 0 needs refine >= 1; ValueError for anything else"""
        if isinstance(lo_rounds, bool) or not isinstance(lo_rounds, (int, np.integer)) or not 0 <= int(lo_rounds) <= 8:
            raise ValueError("lo_rounds is an int 0 .. 8, not %r" % (lo_rounds,))
        if lo_rounds > 0 and int(refine) < 1:
            raise ValueError("lo_rounds >= 1 needs refine >= 1 (a round is `refine` Gauss-Newton steps and a re-selection)")
        return int(lo_rounds)

    def pnp_pair_lo(self, slot_a, slot_b, ratio, K4, lo_rounds, iters=256, thr=1.5, seed=4321, refine=3, want_matches=False, cross_check=False,
                    window=None, loop=None):
        """pnp_pair_window whose refit runs `lo_rounds` (0 .. 8) rounds of {refine steps, re-selection of the inliers under the
        refitted pose} (vo_pnp_pair_lo).  The dict gains lo_rounds (completed) and lo_support (|S_c|); Rt_refined is the LO pose,
        mask the final set S_c, refine_steps the steps of the completed rounds; Rt, best_iter, best_count, q, t stay the RANSAC's."""
        lo_rounds = self.lo_rounds_arg(lo_rounds, refine)
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        head, arrays = self._pnp_out(want_matches)
        lo2 = np.zeros(2, np.int32)
        self._ck(self._lib.vo_pnp_pair_lo(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), _p(K4), int(iters),
                                          float(thr), int(seed) & 0xFFFFFFFF, int(refine), *[_p(a) for a in head + arrays], self.kp_cap, lo_rounds, _p(lo2)))
        return dict(self._pnp_result(head, arrays), lo_rounds=int(lo2[0]), lo_support=int(lo2[1]))

    def pnp_pair_begin_lo(self, slot_a, slot_b, ratio, K4, lo_rounds, iters=256, thr=1.5, seed=4321, refine=3, want_matches=False, cross_check=False,
                          window=None, loop=None):
        """pnp_pair_lo in two halves -> a ticket for pnp_pair_end_lo (or pnp_pair_end, which returns no lo_rounds / lo_support)"""
        lo_rounds = self.lo_rounds_arg(lo_rounds, refine)
        K4 = _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        t = ctypes.c_int(-1)
        self._ck(self._lib.vo_pnp_pair_begin_lo(self._h, int(slot_a), int(slot_b), float(ratio), self._mflags(cross_check, window, loop), _p(K4), int(iters),
                                                float(thr), int(seed) & 0xFFFFFFFF, int(refine), int(bool(want_matches)), lo_rounds, ctypes.byref(t)))
        return t.value

    def pnp_pair_end_lo(self, ticket, want_matches=False):
        head, arrays = self._pnp_out(want_matches)
        lo2 = np.zeros(2, np.int32)
        self._ck(self._lib.vo_pnp_pair_end_lo(self._h, int(ticket), *[_p(a) for a in head + arrays], self.kp_cap, _p(lo2)))
        return dict(self._pnp_result(head, arrays), lo_rounds=int(lo2[0]), lo_support=int(lo2[1]))

    # ---- landmark map (vo_map_*: NOT part of the reference)
    def map_create(self, capacity):
        """-> the handle of a new landmark map of `capacity` landmarks (16 .. kp_cap; at most VO_NUM_MAPS per context)."""
        h = ctypes.c_int(-1)
        self._ck(self._lib.vo_map_create(self._h, int(capacity), ctypes.byref(h)))
        return h.value

    def map_destroy(self, handle):
        self._ck(self._lib.vo_map_destroy(self._h, int(handle)))

    def map_reset(self, handle):
        """size 0, no view, serials start over"""
        self._ck(self._lib.vo_map_reset(self._h, int(handle)))

    @staticmethod
    def _pose12(Rt):
        Rt = np.asarray(Rt, np.float64)
        if Rt.shape == (4, 4):
            Rt = Rt[:3]
        if Rt.size != 12:
            raise ValueError("a pose is 3x4 (or 4x4), not %s" % (Rt.shape,))
        return _c(Rt.reshape(12), np.float64)

    def map_view(self, handle, Rt_cw, K4, z_min, ref_slot, view_slot):
        """The map as seen under the world-to-camera pose Rt_cw (3x4 or 4x4) becomes the keypoints of view_slot, placed in the crop
        of ref_slot's image (vo_map_view).  -> counts2 = [map size, visible]."""
        Rt, K4 = self._pose12(Rt_cw), _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        c2 = np.zeros(2, np.int32)
        self._ck(self._lib.vo_map_view(self._h, int(handle), _p(Rt), _p(K4), float(z_min), int(ref_slot), int(view_slot), _p(c2)))
        return c2

    def map_update(self, handle, slot_new, Rt_wc, serial, max_age, max_obs, q=None, t=None, mask=None):
        """Fold the tracked frame in slot_new (camera-to-world pose Rt_wc) into the map: q / t / mask as pnp_pair(view_slot,
        slot_new, want_matches=True) delivered them, or none of them for insert-and-age only (vo_map_update).
        -> counts6 = [observed, skipped, culled, inserted, dropped, size]."""
        Rt = self._pose12(Rt_wc)
        if q is None and t is None and mask is None:
            q, t, mask = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8)
        elif q is None or t is None or mask is None:
            raise ValueError("q, t and mask come together")
        q, t, mask = _c(q, np.int32).reshape(-1), _c(t, np.int32).reshape(-1), _c(mask, np.uint8).reshape(-1)
        if not len(q) == len(t) == len(mask):
            raise ValueError("q, t and mask differ in length")
        c6 = np.zeros(6, np.int32)
        n = len(q)
        self._ck(self._lib.vo_map_update(self._h, int(handle), int(slot_new), _p(Rt), int(serial), int(max_age), int(max_obs),
                                         _p(q) if n else None, _p(t) if n else None, _p(mask) if n else None, n, _p(c6)))
        return c6

    def map_track(self, handle, slot_new, view_slot, Rt_cw_pred, K4, z_min, ratio, iters, thr, seed, refine, min_matches, max_dist, max_rot,
                  serial, max_age, max_obs, cross_check=False, window=None, loop=None, want_matches=True):
        """The map step in one native call with one synchronisation (vo_track_map): the view of the map under Rt_cw_pred into
        view_slot, the PnP step on (view, slot_new), the odometer's decisions and gates (max_dist / max_rot already scaled by the
        span), and on acceptance the update of the map under the composed pose.  -> the record as a dict (MapTrackRec.as_dict:
        decision, view = counts2, update = counts6, the PnP record, c_T_w / w_T_c 3x4) [+ mask, q, t of length n]."""
        Rt, K4 = self._pose12(Rt_cw_pred), _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        rec = MapTrackRec()
        arrays = [None, None, None]
        if want_matches:
            arrays = self._pnp_out(True)[1]
        self._ck(self._lib.vo_track_map(self._h, int(handle), int(slot_new), int(view_slot), _p(Rt), _p(K4), float(z_min), float(ratio),
                                        self._mflags(cross_check, window, loop), int(iters), float(thr), int(seed) & 0xFFFFFFFF, int(refine),
                                        int(min_matches), float(max_dist), float(max_rot), int(serial), int(max_age), int(max_obs),
                                        ctypes.byref(rec), *[_p(a) for a in arrays], self.kp_cap))
        out = rec.as_dict()
        if want_matches:
            n = out["n"]
            out.update(mask=arrays[0][:n].copy(), q=arrays[1][:n].copy(), t=arrays[2][:n].copy())
        return out

    def track_map_lo(self, handle, slot_new, view_slot, Rt_cw_pred, K4, z_min, ratio, iters, thr, seed, refine, min_matches, max_dist, max_rot,
                     serial, max_age, max_obs, lo_rounds, cross_check=False, window=None, loop=None, want_matches=True):
        """map_track whose PnP step is pnp_pair_lo's (vo_track_map_lo): the decisions, gates and composition see the LO pose, the
        update reads S_c.  The dict gains lo_rounds (completed) and lo_support (|S_c|)."""
        lo_rounds = self.lo_rounds_arg(lo_rounds, refine)
        Rt, K4 = self._pose12(Rt_cw_pred), _c(np.asarray(K4, np.float64).reshape(4), np.float64)
        rec = MapTrackRec()
        arrays = [None, None, None]
        if want_matches:
            arrays = self._pnp_out(True)[1]
        self._ck(self._lib.vo_track_map_lo(self._h, int(handle), int(slot_new), int(view_slot), _p(Rt), _p(K4), float(z_min), float(ratio),
                                           self._mflags(cross_check, window, loop), int(iters), float(thr), int(seed) & 0xFFFFFFFF, int(refine),
                                           int(min_matches), float(max_dist), float(max_rot), int(serial), int(max_age), int(max_obs),
                                           ctypes.byref(rec), *[_p(a) for a in arrays], self.kp_cap, lo_rounds))
        out = dict(rec.as_dict(), lo_rounds=int(rec.pad), lo_support=int(rec.pad2[0]))
        if want_matches:
            n = out["n"]
            out.update(mask=arrays[0][:n].copy(), q=arrays[1][:n].copy(), t=arrays[2][:n].copy())
        return out

    def map_download(self, handle):
        """-> dict(xyz (n, 3) float32 world coordinates, desc (n, 32), octave, obs, last (n,) int32) in map order"""
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_map_download(self._h, int(handle), None, None, None, None, None, 0, ctypes.byref(n)))
        n = n.value
        out = dict(xyz=np.empty((n, 3), np.float32), desc=np.empty((n, 32), np.uint8), octave=np.empty(n, np.int32),
                   obs=np.empty(n, np.int32), last=np.empty(n, np.int32))
        if n:
            self._ck(self._lib.vo_map_download(self._h, int(handle), _p(out["xyz"]), _p(out["desc"]), _p(out["octave"]), _p(out["obs"]),
                                               _p(out["last"]), n, ctypes.byref(ctypes.c_int(0))))
        return out

    def plant_map(self, handle, xyz, desc, rdesc, octave, obs, last):
        """Test-only build of the library: n landmarks straight into a map (vo_test_plant_map).  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_plant_map"):
            raise RuntimeError("plant_map needs the test-only build of the library (libvo355_hooks.so)")
        xyz, desc, rdesc = _c(xyz, np.float32).reshape(-1, 3), _c(desc, np.uint8).reshape(-1, 32), _c(rdesc, np.uint8).reshape(-1, 32)
        octave, obs, last = (_c(a, np.int32).reshape(-1) for a in (octave, obs, last))
        n = len(xyz)
        if not all(len(a) == n for a in (desc, rdesc, octave, obs, last)):
            raise ValueError("one entry of every array per landmark")
        self._ck(self._lib.vo_test_plant_map(self._h, int(handle), n, _p(xyz), _p(desc), _p(rdesc), _p(octave), _p(obs), _p(last)))

    def peek_view(self, handle, slot, n):
        """Test-only build of the library: the first n rows of a view slot's keypoint arrays and of the map's view_src, whatever
        the slot's count says (vo_test_peek_view) -- the padding of map_track's padded view.  The product library has no such entry."""
        if not hasattr(self._lib, "vo_test_peek_view"):
            raise RuntimeError("peek_view needs the test-only build of the library (libvo355_hooks.so)")
        out = dict(xy=np.empty((n, 2), np.float32), xyz=np.empty((n, 3), np.float32), octave=np.empty(n, np.int32),
                   desc=np.empty((n, 32), np.uint8), rdesc=np.empty((n, 32), np.uint8), src=np.empty(n, np.int32))
        self._ck(self._lib.vo_test_peek_view(self._h, int(handle), int(slot), int(n), *[_p(out[k]) for k in ("xy", "xyz", "octave", "desc", "rdesc", "src")]))
        return out

    def umeyama(self, src, dst, force_rotation=True):
        src, dst = _c(src, np.float32).reshape(-1, 3), _c(dst, np.float32).reshape(-1, 3)
        if len(src) != len(dst):
            raise ValueError("Point sets need to have the same size")
        T = np.empty((3, 4), np.float64)
        s = ctypes.c_double(0)
        self._ck(self._lib.vo_umeyama(self._h, _p(src), _p(dst), len(src), int(bool(force_rotation)), _p(T),
                                      ctypes.byref(s)))
        return T, s.value

    def rigid_clique(self, prev, cur, thr):
        prev, cur = _c(prev, np.float32).reshape(-1, 3), _c(cur, np.float32).reshape(-1, 3)
        mask = np.zeros(len(cur), np.int64)
        self._ck(self._lib.vo_rigid_clique(self._h, _p(prev), _p(cur), len(cur), float(thr), _p(mask)))
        return mask

    @staticmethod
    def rodrigues(R):
        R = _c(R, np.float64)
        r = np.empty(3, np.float64)
        lib().vo_rodrigues(_p(R), _p(r))
        return r.reshape(3, 1)

    # ---- instrumentation
    def enable_timing(self, on=True, stages=None):
        """stages: iterable of stage names (T_STAGES) to restrict the event timing to."""
        flag = int(bool(on))
        if on and stages is not None:
            flag = sum(1 << T_STAGES.index(s) for s in stages) << 1
        self._ck(self._lib.vo_enable_timing(self._h, flag))

    def timings(self, reset=False):
        ms = np.zeros(len(T_STAGES), np.float64)
        n = np.zeros(len(T_STAGES), np.int64)
        self._ck(self._lib.vo_get_timings(self._h, _p(ms), _p(n), int(reset)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(T_STAGES)}

    def stage_timeline(self, cap=65536):
        """Development aid: the stage brackets recorded since timings() last resolved them, in the order they were opened, as
        (stage name, entries, begin ms, end ms) relative to the begin of the first (vo_get_stage_timeline).  Consumes nothing;
        empty while timing is off."""
        st, en = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        b, e = np.zeros(cap, np.float64), np.zeros(cap, np.float64)
        n = ctypes.c_int(0)
        self._ck(self._lib.vo_get_stage_timeline(self._h, cap, _p(st), _p(en), _p(b), _p(e), ctypes.byref(n)))
        return [(T_STAGES[st[i]], int(en[i]), float(b[i]), float(e[i])) for i in range(min(n.value, cap))]

    def sgbm_sweep_status(self):
        """Number of SGBM runs of this context whose diagonal sweep gave up a strip hand-off (0 = healthy; sticky).  Results that
        depend on such a run are refused with SweepTimeout where they are picked up."""
        e = ctypes.c_int(0)
        self._ck(self._lib.vo_sgbm_sweep_status(self._h, ctypes.byref(e)))
        return e.value

    def sgbm_sweep_stats(self, block=0, n_words=2048):
        """Control block of the latest aggregation sweep (development aid): see vo_sgbm_sweep_stats."""
        out = np.zeros(n_words, np.int32)
        self._ck(self._lib.vo_sgbm_sweep_stats(self._h, int(block), _p(out), n_words))
        return out

    def measure_copy(self, nbytes=0, reps=20, nontemporal=False):
        """GB/s (read + written) of a streaming device copy between two of the context's volumes."""
        g = ctypes.c_double(0.0)
        self._ck(self._lib.vo_measure_copy(self._h, int(nbytes), int(reps), 1 if nontemporal else 0, ctypes.byref(g)))
        return g.value

    def measure_knn(self, slot_a, slot_b, reps=20, cross_check=False, window=None):
        """microseconds per launch of the Hamming kNN-2 kernel on two slots' descriptors (`reps` launches between two events);
        cross_check=True times the cross-check form of the kernel (with the reset of its column words)."""
        g = ctypes.c_double(0.0)
        self._ck(self._lib.vo_measure_knn_ex(self._h, int(slot_a), int(slot_b), int(reps), self._mflags(cross_check, window), ctypes.byref(g)))
        return g.value

    def shader_clock(self, micros=200):
        """MHz the shader clock holds right now (one wave counting cycles against the 100 MHz wall counter for `micros` us)."""
        g = ctypes.c_double(0.0)
        self._ck(self._lib.vo_shader_clock(self._h, int(micros), ctypes.byref(g)))
        return g.value

    def sgbm_last_geometry(self):
        cells, paths = ctypes.c_int64(0), ctypes.c_int(0)
        self._ck(self._lib.vo_sgbm_last_geometry(self._h, ctypes.byref(cells), ctypes.byref(paths)))
        return cells.value, paths.value
