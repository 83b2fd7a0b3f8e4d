"""StereoOdometer: drop-in for openVO's class (reference stereo_odometer.py:4-226).

Same constructor defaults, class constants, attributes, methods, return values and
`skip_cause` strings.  The per-frame arithmetic (disparity mask + ORB, Hamming kNN + ratio
test, 3-D lookup, rigid-body clique filter, Umeyama fit) runs in libvo355 on the GPU; what
stays in Python is the sequential bookkeeping of `update` -- it decides which frames pair up,
so it follows the reference decision for decision (pinned by tests/golden/g5_state_machine.json).
"""
import collections
import os

import numpy as np

from . import _native
from .features import BFMatcher, DeviceImage, DisparityMask, KeyPointList, ORB


# the loop check's entry in the key of a pose step begun ahead (_pose_params): a type of its own, so that nothing has to guess
# which trailing entry of the key is the match window (a plain (rx, ry) tuple) and which the threshold
LoopCheck = collections.namedtuple("LoopCheck", "max_hamming")
LoRounds = collections.namedtuple("LoRounds", "rounds")          # the marker of pnp_lo_rounds > 0 in _pose_params(): always the last entry
KltTrack = collections.namedtuple("KltTrack", "win levels fb")   # the marker of klt_fused in _pose_params(): the tracker a step was begun with


class StereoOdometer:
    # disparity range (pixels) with a usable depth estimate          [reference :6-7]
    MIN_VALID_DISPARITY = 4
    MAX_VALID_DISPARITY = 100
    # per-frame motion gates, widened by (skipped_frames + 1)          [reference :10,12]
    MAX_DISTANCE_CHANGE = 1          # metres
    MAX_ROTATION_CHANGE = np.pi / 3  # radians

    def __init__(self, stereo_camera, nfeatures=500, match_threshold=0.8, rigidity_threshold=0,
                 outlier_threshold=0, preprocessed_frames=False, min_matches=10,
                 pose_method="umeyama", pnp_iters=256, pnp_threshold=1.5, pnp_seed=4321, cross_check=False, pnp_refine=0,
                 match_window=None, depth="dense", sparse_row_tol=2.0, sparse_max_hamming=75, sparse_mutual=False, sparse_ratio=None,
                 loop_check=None, track="pair", map_max_age=5, map_capacity=None, map_max_obs=8, map_z_min=0.1, map_fused=False,
                 pnp_lo_rounds=0, match="orb", klt_window=21, klt_levels=4, klt_fb=1.0, klt_fused=False,
                 direct_refine=False, direct_levels=3, direct_iters=8, direct_max_points=16384, direct_guard=(0.1, 0.05),
                 direct_affine=False, patch_refine=False, patch_size=5, patch_levels=3, patch_iters=4, patch_guard=(0.1, 0.05)):
        """Arguments up to min_matches are the reference's [reference :14-15].  pose_method="pnp" is an
        extension (not in openVO): the pair's pose comes from RANSAC solvePnP on the previous frame's 3-D
        points and the new frame's keypoint pixels (vo_ransac_pnp) instead of the 3-D/3-D Umeyama fit;
        the rigidity / outlier stages are then not used, the motion gates still apply.
        cross_check=True is an extension too (the reference's "# TODO crosscheck", :21; cv2 itself refuses
        knnMatch(k=2) on a cross-checking matcher): a match must pass the ratio test AND its m[0] must be a mutual
        nearest neighbour (include/vo355.h); every later decision is the reference's, on the smaller set.
        pnp_refine (0 .. 20, pose_method="pnp"): Gauss-Newton steps that refit the RANSAC winner -- the pose of a minimal
        sample -- on its whole inlier set, as cv2.solvePnPRansac's final fit does; 0 (default) returns the winner itself, 3 is
        the recommended value.  The refinement is part of the fused device step (vo_pnp_pair): where that step cannot run
        (_pair_pnp: a replaced matcher or seam -- the context's point_clouds / ransac_pnp replaced on the object count as
        seams of this mode --, more than 3800 keypoints) the winner is returned as it is.
        match_window (None, a radius, or (rx, ry) in pixels; an extension, the reference's "# TODO config" at its match step,
        :165): a keypoint of the older frame is matched only against keypoints of the newer one no farther than rx in x and ry
        in y (include/vo355.h).  The radii are per frame: like the motion gates they are multiplied by the frames the pair
        spans -- skipped_frames + 1 for (current, next), skipped_frames + 2 for the one-frame-back fallback.  A keypoint with
        fewer than two candidates in its window gives no match, and the ratio test inside a window is laxer than over the
        whole image: the window replaces the clique filter on the default odometer, it does not add to it (README).
        depth="sparse" (an extension; default "dense" = the reference's path): no disparity image is computed.  ORB runs on both
        rectified images, left and right keypoints are associated along the row (at most sparse_row_tol pixels apart in y at
        the keypoint's scale, Hamming distance at most sparse_max_hamming) and refined to sub-pixel (StereoCamera.compute_sparse,
        include/vo355.h); a frame's keypoints are then the left keypoints that have a depth, current_3d / prev_3d are their (n, 3)
        points and current_disparity their (n,) disparities.  The state machine, both pose methods, cross_check and match_window
        are unchanged; feature_mask is not used.  run() submits sparse pairs ahead like dense ones (StereoCamera.submit_sparse): their
        upload, both extractions, association and compaction run on the look-ahead engines, update() collects.
        sparse_mutual / sparse_ratio (depth="sparse" only; off by default): two tests on the left/right association
        (include/vo355.h, vo_set_sparse_assoc) -- a right keypoint belongs to its best left claimant only; the winner's Hamming
        distance must be below sparse_ratio (0 < ratio <= 1) times the runner-up's.  They are part of the sparse request: update(),
        run() and the pairs begun ahead all carry them.
        loop_check (None, or a Hamming threshold 0 .. 256; depth="sparse" only): the circular check of sparse stereo odometry -- a
        temporal match (q, t) is kept only when the RIGHT-image partners of q and t are within loop_check bits of each other
        (include/vo355.h, VO_MATCH_LOOP).  Applied after the ratio test, cross_check and match_window, in update() and run(),
        with both pose methods and on the one-frame-back fallback; the threshold is not scaled with the frames a pair spans.  The
        generic path (a replaced matcher or seam) applies the same test on KeypointDepth.right_desc.
        track="map" (an extension, NOT in the reference; default "pair" = every pose is the pose of one pair of frames, as ever;
        needs depth="sparse" and pose_method="pnp"): the new frame is tracked against a landmark map resident on the device
        (include/vo355.h, vo_map_*).  The map as seen under the last pose becomes one more depth-carrying frame slot (the VIEW: the
        camera sets a slot aside for it), the fused PnP step runs on (view, new frame) and its result goes through exactly the
        decisions and gates of the pairwise step; an accepted frame is folded into the map: matched inliers update their landmark's
        position by a running mean (weight never below 1 / (map_max_obs + 1)) and take the new descriptors, unmatched keypoints
        enter as landmarks, landmarks not observed for more than map_max_age accepted frames leave.  When the map step gives no
        pose, today's two pairwise attempts run unchanged and the frame enters the map without observations; track_source says
        which of the two ("map" | "pair") placed the last accepted frame, map_counts holds the last counts of view / update,
        landmarks() downloads the map.  map_capacity: None = min(kp_cap, 4 * nfeatures); map_z_min: landmarks nearer than this
        (metres along the optical axis) are not in a view.  cross_check, match_window (a guided search around the landmark's
        predicted pixel, scaled by the span as ever), pnp_refine and loop_check compose unchanged.  No pose step is begun ahead in
        this mode; run() still submits sparse pairs ahead.  Where the fused PnP step cannot run (a replaced matcher or seam),
        update() raises ValueError.
        map_fused=True (track="map" only; default False): the map step -- view, PnP step, decisions, motion gates, pose composition
        and the update of the map -- is ONE native call with one device synchronisation (vo_track_map) instead of three calls with
        the host's arithmetic between them.  The decisions and counts are those of the unfused chain; c_T_w comes from the device
        (composed and inverted there in a fixed order: equal to the host's to the last bits, not bit for bit).  A frame that finds
        more than 3800 landmarks in the map takes the unfused chain.
        pnp_lo_rounds (0 .. 8; default 0 = the refit as above; a value above 0 needs pose_method="pnp" and pnp_refine >= 1):
        local-optimisation rounds of the fused PnP step (LO-RANSAC; include/vo355.h, vo_pnp_pair_lo).  A round is pnp_refine
        Gauss-Newton steps on the present inlier set, then the re-selection of that set under the refitted pose by the scoring
        kernels' own test; a round that cannot run (fewer than 6 points, a failed solve) is discarded and ends the loop.  One
        round is today's refit; 3 is the value the tables of DESIGN were made with.  The decisions are unchanged: "outlier" still
        reads the RANSAC winner's count, the gates see the LO pose.  With track="map" the final set is what updates the map.  It
        is part of the key of a step begun ahead.  Where the fused step cannot run, the winner is returned as it is, as with
        pnp_refine.  pnp_lo_counts = (rounds completed, support) of the last fused step.
        match="klt" (an extension, NOT in the reference; default "orb" = every temporal association is a descriptor match, as ever):
        the keypoints of the older frame are TRACKED into the newer frame's rectified left image by pyramidal Lucas-Kanade with a
        forward-backward check (include/vo355.h, vo_klt_track) instead of being matched against its descriptors: klt_window (odd,
        5 .. 31) is the window, klt_levels (1 .. 6) the pyramid levels, klt_fb the forward-backward radius in pixels (0: no check).
        A track with a non-zero status is dropped; fewer than min_matches tracks: skip_cause "matches".  pose_method="pnp": the
        3-D points of the older frame at its own keypoints and the tracked sub-pixel positions go through vo_ransac_pnp and the
        decisions of the composed PnP path; pose_method="umeyama" (depth="dense" only: a tracked position is no keypoint of the
        newer frame, so only a dense disparity has a depth for it): the newer frame's 3-D points are looked up at the tracked
        positions and point_cloud_transform runs unchanged.  A track whose 3-D lookup in either frame has no usable tap or no finite
        point, or which has left the crop, is DROPPED (the keypoint paths raise ZeroDivisionError there).  The new frame's ORB
        extraction still runs: its keypoints are what the next pair tracks.  Both frames must be on the device (ValueError
        otherwise, as with pose_method="pnp"); no pose step is begun ahead (but see klt_fused), run() still submits pairs ahead; the one-frame-back
        fallback takes the same path.  cross_check, match_window, loop_check and track="map" belong to the descriptor matcher and
        are refused with match="klt".  klt_counts = (keypoints tracked from, tracks kept) of the last pair.
        klt_fused=True (match="klt" with pose_method="pnp" only; default False): the pair step -- tracking, the filter, the 3-D lookup
        and the RANSAC -- is ONE native call with one synchronisation (vo_klt_pnp_pair) instead of three or four, nothing per
        keypoint comes back, and steps are begun ahead on pairs that are already on the device, as with match="orb"
        (_start_next_pose; klt_ahead counts the steps collected from a ticket begun ahead).  The decisions are those of the
        composed path in its order; with pnp_refine / pnp_lo_rounds the gates see the refined pose where the refit succeeded (the
        composed path does not refine).  Admitted per pair like the fused PnP step -- an exact StereoOdometer, no replaced seam,
        frames on the device, at most 3800 keypoints in the older frame; otherwise the composed path runs.
        direct_refine=True (an extension, NOT in the reference; default False; needs depth="dense"): every pose a pair step has
        produced -- either pose method, match="orb" or "klt", the one-frame-back fallback too -- is handed, BEFORE the motion
        gates, to the dense direct alignment (include/vo355.h, vo_direct_align) as its start: the older frame's rectified left image
        and whole disparity against the newer frame's image, direct_levels pyramid levels (1 .. 4), direct_iters iterations per
        level (1 .. 20), at most direct_max_points lattice points per level, the odometer's valid-disparity range.  The refined pose
        replaces the feature pose iff the step ended with status 0 and moved it by no more than direct_guard = (metres, radians),
        scaled by skipped_frames + 1 like the gates; otherwise the feature pose stands.  direct_status is the status of the last
        step, direct_record its whole record, direct_accepted whether its pose was taken, pose_information the 6 x 6 information
        matrix (rotation, then translation; up to the noise scale) of the pose the last step delivered: None whenever that step's
        pose was not taken or the motion gates refused it (never the matrix of an older pose).  The call is synchronous, under
        run() as well: one more synchronisation per frame.  Both frames must be on the device (ValueError otherwise).
        The guard has to be at least as wide as the feature pose's own error, or it refuses exactly the corrections that matter.
        The default is sized for pose_method="pnp", whose poses are centimetres off.  With pose_method="umeyama" WIDEN IT: the
        3-D / 3-D fit can be decimetres off per pair, the default guard then refuses most refined poses, and a chain in which
        only some pairs are corrected can end farther from the truth than the unrefined one (measured on the synthetic corridor
        T0: 0.3655 m against 0.3197 m unrefined with the default guard, 0.0025 m with direct_guard=(0.5, 0.1)).
        direct_affine=True (default False; read only with direct_refine=True; needs direct_iters >= 3): the alignment estimates a
        gain and an offset of the newer image's brightness beside the pose (vo_direct_align_ab), for streams whose exposure moves
        between frames: the plain alignment assumes brightness constancy and walks away from the pose when it does not hold.
        direct_brightness is (gain, offset) of the last step, None when that step completed fewer than three iterations (none that estimates them);
        pose_information is then the pose information marginalised over the brightness.  Guard, gates and status handling are
        unchanged.
        patch_refine=True (an extension, NOT in the reference; default False; needs depth="sparse" and track="pair"; not together
        with direct_refine): the photometric refinement for sparse stereo depth.  Every pose that reaches the motion gates --
        either pose method, match="orb" or "klt" (klt_fused included), the one-frame-back fallback too -- is first handed to the
        PATCH alignment (include/vo355.h, vo_direct_align_kp) as its start: a patch_size x patch_size pixel patch (3, 5 or 7)
        around every keypoint of the older frame, each pixel at its keypoint's sparse depth, against the newer frame's rectified
        left image, patch_levels pyramid levels (1 .. 4), patch_iters iterations per level (1 .. 20).  No disparity image is
        computed.  The refined pose replaces the feature pose iff the step ended with status 0 and moved it by no more than
        patch_guard = (metres, radians), scaled by skipped_frames + 1: direct_refine's rule exactly, and what is said there about
        the guard and pose_method="umeyama" holds here.  patch_status is the status of the last step, patch_record its whole record,
        patch_accepted whether its pose was taken, pose_information the 6 x 6 information matrix of the pose the last step
        delivered: None whenever that pose was not taken or the gates refused it.  The call is synchronous, under run() as well:
        one more synchronisation per frame.  Both frames must be on the device (ValueError otherwise).  track="map" is refused:
        the view slot holds no image."""
        if not isinstance(track, str) or track not in ("pair", "map"):
            raise ValueError("track must be 'pair' or 'map'")
        if track == "map" and (depth != "sparse" or pose_method != "pnp"):
            raise ValueError("track='map' needs depth='sparse' and pose_method='pnp'")
        if not isinstance(map_fused, (bool, np.bool_)):
            raise ValueError("map_fused must be True or False")
        if map_fused and track != "map":
            raise ValueError("map_fused=True needs track='map'")
        if map_fused:                # (an instance attribute only where the option is on: without it the object is what it was)
            self.map_fused = True

        def _int(v, lo, hi):
            return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and lo <= v <= hi
        if not _int(map_max_age, 0, 2 ** 31 - 1):
            raise ValueError("map_max_age must be an int >= 0")
        if not _int(map_max_obs, 1, 65535):
            raise ValueError("map_max_obs must be an int in 1 .. 65535")
        kp_cap = getattr(getattr(stereo_camera, "_ctx", None), "kp_cap", 2 ** 31 - 1)
        if map_capacity is not None and not _int(map_capacity, 16, kp_cap):
            raise ValueError("map_capacity must be None or an int in 16 .. kp_cap (%d)" % kp_cap)
        with np.errstate(over="ignore"):               # (too large for float32: inf, refused)
            if (isinstance(map_z_min, (bool, np.bool_)) or not isinstance(map_z_min, (int, float, np.integer, np.floating))
                    or not np.isfinite(np.float32(map_z_min)) or map_z_min < 0):
                raise ValueError("map_z_min must be a finite number >= 0")
        self.track, self.map_max_age, self.map_max_obs, self.map_z_min = track, int(map_max_age), int(map_max_obs), float(map_z_min)
        self.map_capacity = None if map_capacity is None else int(map_capacity)
        self.track_source = None     # "map" | "pair": what placed the last accepted frame (track="map")
        self.map_counts = {}         # {"view": counts2, "update": counts6} of the last map calls
        self._map = self._view_slot = None
        self._map_serial = 0
        if not isinstance(depth, str) or depth not in ("dense", "sparse"):
            raise ValueError("depth must be 'dense' or 'sparse'")
        if (isinstance(sparse_row_tol, (bool, np.bool_)) or not isinstance(sparse_row_tol, (int, float, np.integer, np.floating))
                or not np.isfinite(sparse_row_tol) or sparse_row_tol < 0):
            raise ValueError("sparse_row_tol must be a finite number >= 0")
        if (isinstance(sparse_max_hamming, (bool, np.bool_)) or not isinstance(sparse_max_hamming, (int, np.integer))
                or not 0 <= sparse_max_hamming <= 256):
            raise ValueError("sparse_max_hamming must be an int in 0 .. 256")
        self.depth, self.sparse_row_tol, self.sparse_max_hamming = depth, float(sparse_row_tol), int(sparse_max_hamming)
        try:
            _native.sparse_assoc_state(sparse_mutual, sparse_ratio)
        except ValueError as e:
            raise ValueError("sparse_mutual / sparse_ratio: %s" % e)
        if depth == "dense" and (sparse_mutual or sparse_ratio is not None):
            raise ValueError("sparse_mutual / sparse_ratio need depth='sparse'")
        self.sparse_mutual, self.sparse_ratio = bool(sparse_mutual), None if sparse_ratio is None else float(sparse_ratio)
        self.loop_check = _native.loop_threshold(loop_check, "loop_check")
        if depth == "dense" and self.loop_check is not None:
            raise ValueError("loop_check needs depth='sparse'")
        if pose_method not in ("umeyama", "pnp"):
            raise ValueError("pose_method must be 'umeyama' or 'pnp'")
        if not isinstance(cross_check, (bool, np.bool_)):
            raise ValueError("cross_check must be True or False")
        self.cross_check = bool(cross_check)
        self.match_window = _native.window_radii(match_window, "match_window")
        self._pair_span = None       # frames the pair being tried spans (_try_pair); None: skipped_frames + 1
        if not isinstance(match, str) or match not in ("orb", "klt"):
            raise ValueError("match must be 'orb' or 'klt'")
        try:
            klt = _native.Context.klt_params(win=klt_window, levels=klt_levels, fb=klt_fb)
        except ValueError as e:
            raise ValueError("klt_window / klt_levels / klt_fb: %s" % e)
        if match == "klt":
            if depth == "sparse" and pose_method == "umeyama":
                raise ValueError("match='klt' with depth='sparse' needs pose_method='pnp' (a tracked position has no sparse depth)")
            if track == "map":
                raise ValueError("match='klt' needs track='pair'")
            if self.cross_check or self.match_window is not None or self.loop_check is not None:
                raise ValueError("cross_check, match_window and loop_check belong to the descriptor matcher: not with match='klt'")
            # (instance attributes only where the option is on: without it the object is what it was)
            self.match, self.klt_window, self.klt_levels, self.klt_fb = "klt", klt[0], klt[1], klt[5]
            self.klt_counts = None
        if not isinstance(klt_fused, (bool, np.bool_)):
            raise ValueError("klt_fused must be True or False")
        if klt_fused and (match != "klt" or pose_method != "pnp"):
            raise ValueError("klt_fused=True needs match='klt' and pose_method='pnp'")
        if klt_fused:                # (instance attributes only where the option is on: without it the object is what it was)
            self.klt_fused = True
            self.klt_ahead = 0       # pair steps collected from a ticket begun ahead
        if isinstance(pnp_refine, (bool, np.bool_)) or not isinstance(pnp_refine, (int, np.integer)) or not 0 <= pnp_refine <= 20:
            raise ValueError("pnp_refine must be an int in 0 .. 20")
        self.pnp_refine = int(pnp_refine)
        if isinstance(pnp_lo_rounds, (bool, np.bool_)) or not isinstance(pnp_lo_rounds, (int, np.integer)) or not 0 <= pnp_lo_rounds <= 8:
            raise ValueError("pnp_lo_rounds must be an int in 0 .. 8")
        if pnp_lo_rounds > 0 and (pose_method != "pnp" or self.pnp_refine < 1):
            raise ValueError("pnp_lo_rounds > 0 needs pose_method='pnp' and pnp_refine >= 1")
        if pnp_lo_rounds > 0:        # (instance attributes only where the option is on: without it the object is what it was)
            self.pnp_lo_rounds = int(pnp_lo_rounds)
            self.pnp_lo_counts = None
        if not isinstance(direct_refine, (bool, np.bool_)):
            raise ValueError("direct_refine must be True or False")
        if direct_refine:
            if depth != "dense":
                raise ValueError("direct_refine=True needs depth='dense' (the alignment reads a dense disparity)")
            try:
                prm = _native.Context.direct_params(levels=direct_levels, iters=direct_iters, max_points=direct_max_points,
                                                    dmin=self.MIN_VALID_DISPARITY, dmax=self.MAX_VALID_DISPARITY)
                guard = tuple(direct_guard)
                if len(guard) != 2 or any(isinstance(g, (bool, np.bool_, str, bytes)) or not np.isfinite(g) or g < 0 for g in guard):
                    raise TypeError
            except ValueError as e:
                raise ValueError("direct_levels / direct_iters / direct_max_points: %s" % e)
            except TypeError:
                raise ValueError("direct_guard is a pair (metres, radians) of finite numbers >= 0, not %r" % (direct_guard,))
            # (instance attributes only where the option is on: without it the object is what it was)
            self.direct_refine = True
            self.direct_levels, self.direct_iters, self.direct_max_points = prm[0], prm[1], prm[2]
            self.direct_guard = (float(guard[0]), float(guard[1]))
            self.direct_status = self.direct_record = self.pose_information = None
            self.direct_accepted = False
            self._direct_pair = None     # (slot a, slot b) of the pair being tried, None while its frames are not on the device
            if not isinstance(direct_affine, (bool, np.bool_)):
                raise ValueError("direct_affine must be True or False")
            if direct_affine:
                if self.direct_iters < 3:
                    raise ValueError("direct_affine=True needs direct_iters >= 3 (the first two iterations of a level hold the brightness)")
                self.direct_affine = True        # (instance attributes only in affine mode, as above)
                self.direct_brightness = None
        if not isinstance(patch_refine, (bool, np.bool_)):
            raise ValueError("patch_refine must be True or False")
        if patch_refine:
            if depth != "sparse":
                raise ValueError("patch_refine=True needs depth='sparse' (the alignment reads the keypoints' sparse depth; direct_refine is the dense one)")
            if track == "map":
                raise ValueError("patch_refine=True needs track='pair' (the view slot of track='map' holds no image)")
            if direct_refine:
                raise ValueError("patch_refine=True and direct_refine=True exclude each other")
            try:
                prm = _native.Context.direct_kp_params(levels=patch_levels, iters=patch_iters, patch=patch_size)
                guard = tuple(patch_guard)
                if len(guard) != 2 or any(isinstance(g, (bool, np.bool_, str, bytes)) or not np.isfinite(g) or g < 0 for g in guard):
                    raise TypeError
            except ValueError as e:
                raise ValueError("patch_levels / patch_iters / patch_size: %s" % e)
            except TypeError:
                raise ValueError("patch_guard is a pair (metres, radians) of finite numbers >= 0, not %r" % (patch_guard,))
            # (instance attributes only where the option is on: without it the object is what it was)
            self.patch_refine = True
            self.patch_levels, self.patch_iters, self.patch_size = prm[0], prm[1], prm[2]
            self.patch_guard = (float(guard[0]), float(guard[1]))
            self.patch_status = self.patch_record = self.pose_information = None
            self.patch_accepted = False
            self._patch_pair = None      # (slot a, slot b) of the pair being tried, None while its frames are not on the device
        self.pose_method, self.pnp_iters, self.pnp_threshold, self.pnp_seed = pose_method, pnp_iters, pnp_threshold, pnp_seed
        self.stereo = stereo_camera
        self.current_img = self.current_disparity = self.current_3d = None
        self.prev_img = self.prev_disparity = self.prev_3d = None
        ctx = getattr(stereo_camera, "_ctx", None)
        self._ctx = ctx
        self.orb = ORB(ctx, nfeatures) if ctx is not None else None
        self.matcher = BFMatcher(ctx) if ctx is not None else None
        self.prev_kps = self.current_kps = None
        self.current_desc = None
        self.match_threshold = match_threshold
        self.rigidity_threshold = rigidity_threshold
        self.outlier_threshold = outlier_threshold
        self.preprocessed_frames = preprocessed_frames
        self.min_matches = min_matches
        self.skipped_frames = 0      # successive frames without an accepted transform
        self.c_T_w = np.eye(4)       # world frame expressed in the camera frame
        self.c_T_w_prev = np.eye(4)
        self.skip_cause = ""
        self._specs = {}             # (slot key a, slot key b, params) -> ticket of a pose step started ahead of time
        self._next_hint = ()         # SubmittedPairs expected by the next update() calls (set by run())
        self._ahead_counts = {}      # (slot, generation), ORB arguments -> keypoint count of a look-ahead pair already collected
        self.pose_ahead = max(0, min(int(os.environ.get("VO_POSE_AHEAD", "4")), _native.VO_NUM_POSE_ASYNC - 1))   # 4 against 6 / 5 / 3 / 2: DESIGN 4b

    # ------------------------------------------------------------------------------------------
    def feature_mask(self, disparity):
        """uint8 {0,255} mask of MIN_VALID_DISPARITY <= d <= MAX_VALID_DISPARITY  [reference :38-41].
        For a device-resident disparity the mask is returned unevaluated and fused into ORB."""
        if isinstance(disparity, DeviceImage) and disparity.kind == "disp" and disparity.frame.live:
            return DisparityMask(disparity.frame, self.MIN_VALID_DISPARITY, self.MAX_VALID_DISPARITY)
        d = np.asarray(disparity)
        return ((d >= self.MIN_VALID_DISPARITY) * (d <= self.MAX_VALID_DISPARITY)).astype(np.uint8) * 255

    def valid_distance_change(self, prev_kp_idx, current_kp_idx):
        """Unused by the reference (guarded by `if (False)`, :165-166); kept for API parity [:43-48]."""
        p_x, p_y = self.prev_kps[prev_kp_idx].pt
        c_x, c_y = self.current_kps[current_kp_idx].pt
        a = np.linalg.norm(np.asarray(self.prev_3d)[int(p_y)][int(p_x)])
        b = np.linalg.norm(np.asarray(self.current_3d)[int(c_y)][int(c_x)])
        return a - b <= self.MAX_DISTANCE_CHANGE * (self.skipped_frames + 1)

    def bilinear_interpolate_pixels(self, img, x, y):
        """Inf-aware bilinear sample of an HxWx3 image at float (x, y)  [reference :50-79].
        Raises ZeroDivisionError when no tap is usable, like the reference."""
        if isinstance(img, DeviceImage) and img.kind == "xyz" and img.frame.live:
            out, st = self._ctx.points3d_at(img.frame.slot, np.array([[x, y]], np.float32))
        else:
            out, st = self._ctx.bilinear_at(np.asarray(img, np.float32), np.array([[x, y]], np.float32))
        if st[0] == 2:
            raise ZeroDivisionError("division by zero")
        return out[0]

    def rigid_body_filter(self, prev_pts, pts):
        """Greedy maximum clique of pairwise-distance-consistent matches  [reference :82-105]."""
        return self._ctx.rigid_clique(np.asarray(prev_pts, np.float32), np.asarray(pts, np.float32),
                                      self.rigidity_threshold)

    def save_frame_update(self, next_img, next_disp, next_3d, next_kps, next_desc):
        self.prev_img, self.prev_disparity, self.prev_3d = self.current_img, self.current_disparity, self.current_3d
        self.prev_kps, self.prev_desc = self.current_kps, self.current_desc
        self.current_img, self.current_disparity, self.current_3d = next_img, next_disp, next_3d
        self.current_kps, self.current_desc = next_kps, next_desc

    # ------------------------------------------------------------------------------------------
    def update(self, img_left, img_right):
        """Process one stereo pair; True when the frame was accepted  [reference :115-160].

        Raises _native.SweepTimeout (a VoError) instead of returning when the pair's disparity is undefined -- a strip
        hand-off inside its aggregation sweep gave up waiting on an oversubscribed GPU: no pose is ever derived from such a
        pair.  The odometer's state is that of before the call (the frame is neither saved nor counted as skipped); the same
        pair may be passed again, or the next one."""
        if self.depth == "sparse":
            # (the association keywords only where a test is on: a camera stand-in with the earlier signature keeps working)
            assoc = dict(mutual=self.sparse_mutual, assoc_ratio=self.sparse_ratio) if self.sparse_mutual or self.sparse_ratio is not None else {}
            next_kps, next_desc, next_3d, next_disp, next_img = self.stereo.compute_sparse(
                img_left, img_right, self.orb.nfeatures, preprocessed=self.preprocessed_frames, min_disp=self.MIN_VALID_DISPARITY,
                max_disp=self.MAX_VALID_DISPARITY, row_tol=self.sparse_row_tol, max_hamming=self.sparse_max_hamming, **assoc)
            if self.loop_check is not None and isinstance(next_3d, DeviceImage):
                next_3d.frame.keep_rdesc = True         # (the right partners' descriptors stay with a frame that leaves the device)
        else:
            next_3d, next_disp, next_img = self.stereo.compute_3d(img_left, img_right,
                                                                  preprocessed=self.preprocessed_frames)
            next_kps, next_desc = self.orb.detectAndCompute(next_img, self.feature_mask(next_disp))
        if len(next_kps) < self.min_matches:
            self.skipped_frames += 1
            self.skip_cause = "keypoints"
            return False
        if self.current_img is None:           # very first usable frame
            if self.track == "map":
                self._map_first(next_kps, next_desc, next_3d)
            self.save_frame_update(next_img, next_disp, next_3d, next_kps, next_desc)
            return True

        if self.track == "map" and self._map_track(next_kps, next_desc, next_3d):
            self.skipped_frames = 0
            self.save_frame_update(next_img, next_disp, next_3d, next_kps, next_desc)
            return True

        # (the span is passed only where a window needs it: a subclass that replaces _try_pair keeps the signature it has)
        span = {} if self.match_window is None else {"span": self.skipped_frames + 1}
        T = self._try_pair(self.current_kps, self.current_desc, self.current_3d, next_kps, next_desc, next_3d, **span)
        if T is not None:
            self.c_T_w_prev = self.c_T_w
            self.c_T_w = T @ self.c_T_w
        elif self.prev_img is not None:
            # one-frame-back fallback: pair the new frame with the frame before `current`
            span = {} if self.match_window is None else {"span": self.skipped_frames + 2}
            T = self._try_pair(self.prev_kps, self.prev_desc, self.prev_3d, next_kps, next_desc, next_3d, **span)
            if T is not None:
                base = self.c_T_w_prev
                self.c_T_w_prev = self.c_T_w
                self.c_T_w = T @ base
                self.skipped_frames = 0
        if T is None:
            self.skipped_frames += 1          # frame is dropped, `current` stays
            return False
        self.skipped_frames = 0
        if self.track == "map":                # placed by a pairwise attempt: the frame enters the map without observations
            self._map_fold(next_kps.frame.slot)
            self.track_source = "pair"
        self.save_frame_update(next_img, next_disp, next_3d, next_kps, next_desc)
        self._start_next_pose()
        return True

    # ---- frame-to-map tracking (track="map") ------------------------------------------------------------------------------------
    def _map_ready(self, kps, desc, im3d):
        """The map step is the fused PnP step on device-resident slots: where that cannot run there is no map mode.  Creates the
        map and takes the view slot at first use."""
        if not (type(self) is StereoOdometer and type(self.matcher) is BFMatcher and self._pnp_fused_ok()
                and not any(n in self.__dict__ for n in self._SEAMS) and self._on_device(kps, desc, im3d)):
            raise ValueError("track='map' needs the fused PnP step on device-resident frames: a replaced matcher or seam "
                             "(or a frame that has left the device) leaves it nothing to run on")
        if self._map is None:
            cap = self.map_capacity if self.map_capacity is not None else min(self._ctx.kp_cap, 4 * self.orb.nfeatures)
            self._map = self._ctx.map_create(max(16, cap))
        if self._view_slot is None:
            self._view_slot = self.stereo.reserve_view_slot()

    def _map_first(self, kps, desc, im3d):
        """the first usable frame: an empty map, the frame enters it with the identity pose and serial 0"""
        self._map_ready(kps, desc, im3d)
        self._ctx.map_reset(self._map)
        self._map_serial = 0
        self.track_source = None
        self._map_fold(kps.frame.slot)

    def _map_fold(self, slot, r=None):
        """the frame in `slot`, placed at c_T_w, into the map (r: the PnP record of the map step, or None = no observations)"""
        m = (r["q"], r["t"], r["mask"]) if r is not None else (None, None, None)
        self.map_counts["update"] = self._ctx.map_update(self._map, slot, np.linalg.inv(self.c_T_w), self._map_serial, self.map_max_age,
                                                         self.map_max_obs, *m)
        self._map_size = int(self.map_counts["update"][5])
        self._map_serial += 1

    def _map_track(self, kps, desc, im3d):
        """The map step: view under c_T_w (the prediction is the last pose) -> fused PnP step on (view, new frame) -> the decisions
        of _pair_pnp_fused -> c_T_w and the map updated.  -> True when the frame was placed."""
        self._map_ready(kps, desc, im3d)
        slot = kps.frame.slot
        Q = self.stereo.Q
        K4 = (float(Q[2, 3]), float(Q[2, 3]), float(-Q[0, 3]), float(-Q[1, 3]))
        if self.map_fused and len(kps) >= 2 and self._map_size <= _native.MAP_TRACK_MAX:
            return self._map_track_fused(slot, K4)
        c2 = self.map_counts["view"] = self._ctx.map_view(self._map, self.c_T_w, K4, self.map_z_min, slot, self._view_slot)
        if not (max(self.min_matches, 2) <= int(c2[1]) <= 3800 and len(kps) >= 2):
            return False
        got = {}
        self._pair_span = None
        T = self._pair_pnp_fused(self._view_slot, slot, want_matches=True, record=got)
        if T is None:
            return False
        self.c_T_w_prev = self.c_T_w
        self.c_T_w = T @ self.c_T_w
        self._map_fold(slot, got["r"])
        self.track_source = "map"
        return True

    def _map_track_fused(self, slot, K4):
        """_map_track in one native call (vo_track_map): the same decisions in the same order, taken on the device."""
        self._pair_span = None
        span = self.skipped_frames + 1
        kw = self._pnp_kwargs(self._pose_params())
        args = (self._map, slot, self._view_slot, self.c_T_w, K4, self.map_z_min, kw["ratio"], kw["iters"], kw["thr"], kw["seed"], kw["refine"],
                self.min_matches, self.MAX_DISTANCE_CHANGE * span, self.MAX_ROTATION_CHANGE * span, self._map_serial, self.map_max_age,
                self.map_max_obs)
        more = dict(cross_check=kw["cross_check"], window=kw.get("window"), loop=kw.get("loop"), want_matches=False)
        if "lo_rounds" in kw:
            r = self._ctx.track_map_lo(*args, kw["lo_rounds"], **more)
            self.pnp_lo_counts = (r["lo_rounds"], r["lo_support"])
        else:
            r = self._ctx.map_track(*args, **more)
        self.map_counts["view"] = r["view"]
        if r["flags"] & 1 and r["decision"] not in (1, 2):     # (behind the view and the match count, as in _pair_pnp_fused)
            raise ZeroDivisionError("division by zero")
        cause = _native.MAP_DECISIONS[r["decision"]]
        if r["decision"] != 0:
            if cause is not None:
                self.skip_cause = cause
            return False
        self.c_T_w_prev = self.c_T_w
        self.c_T_w = np.vstack([r["c_T_w"], [0, 0, 0, 1]])
        self.map_counts["update"] = r["update"]
        self._map_size = int(r["update"][5])
        self._map_serial += 1
        self.track_source = "map"
        return True

    def landmarks(self):
        """-> the map as a dict of arrays in map order: xyz (n, 3) float32 world coordinates (the camera frame of the first tracked
        frame), desc (n, 32), octave, obs, last (n,); empty before the first frame (track="map" only)"""
        if self.track != "map":
            raise ValueError("landmarks() needs track='map'")
        if self._map is None:
            return dict(xyz=np.zeros((0, 3), np.float32), desc=np.zeros((0, 32), np.uint8), octave=np.zeros(0, np.int32),
                        obs=np.zeros(0, np.int32), last=np.zeros(0, np.int32))
        return self._ctx.map_download(self._map)

    def release_map(self):
        """Give the map and the view slot back (idempotent; also done when the odometer is collected)."""
        ctx, cam = self._ctx, self.stereo
        if self._map is not None and ctx is not None and getattr(ctx, "_h", None):
            try:
                ctx.map_destroy(self._map)
            except _native.VoError:
                pass
        self._map = None
        if self._view_slot is not None and hasattr(cam, "release_view_slot"):
            cam.release_view_slot(self._view_slot)
        self._view_slot = None

    def __del__(self):
        try:
            if self.__dict__.get("_map") is not None or self.__dict__.get("_view_slot") is not None:
                self.release_map()
        except Exception:
            pass

    match = "orb"            # "klt" (constructor): pairs are associated by Lucas-Kanade tracking (_pair_klt)
    klt_fused = False        # True (constructor): the Lucas-Kanade pair step is one native call (_pair_klt_fused)
    _KLT_CTX_SEAMS = ("klt_track", "points3d_at", "ransac_pnp")
    pnp_lo_rounds = 0        # 1 .. 8 (constructor): local-optimisation rounds of the fused PnP step (the _lo entries are called)
    pnp_lo_counts = None     # (rounds completed, support) of the last fused step with pnp_lo_rounds > 0
    map_fused = False        # True (constructor): the map step is one native call (_map_track_fused)
    direct_refine = False    # True (constructor): every pair pose goes through the dense direct alignment before the gates (_direct)
    direct_affine = False    # True (constructor): the alignment estimates a gain and an offset of the newer image beside the pose
    direct_brightness = None  # (gain, offset) of the last step in affine mode; None when the step gave none
    patch_refine = False     # True (constructor): every pair pose goes through the patch alignment before the gates (_patch)
    _map_size = 0            # landmarks in the map as its last update reported (set with the first fold)
    _pnp_fused = True        # False: pose_method="pnp" takes the composed path (_pair_pnp) whatever the conditions
    _PNP_CTX_SEAMS = ("point_clouds", "ransac_pnp")

    def _pnp_fused_ok(self):
        """The two native calls the composed PnP path is made of are seams too: replaced on the context object (instrumented,
        say), they are what runs, so the fused step -- which would bypass them -- stands back."""
        return self._pnp_fused and not any(n in getattr(self._ctx, "__dict__", {}) for n in self._PNP_CTX_SEAMS)

    def _klt_fused_ok(self):
        """as _fused_ok for the Lucas-Kanade step: the three native calls the composed path is made of are its seams"""
        return (self.klt_fused and type(self) is StereoOdometer and not any(n in self.__dict__ for n in self._SEAMS)
                and not any(n in getattr(self._ctx, "__dict__", {}) for n in self._KLT_CTX_SEAMS))

    def _window(self, span=None):
        """The match window of a pair that spans `span` frames (None: the pair being tried, else skipped_frames + 1): the radii
        as the float32 values the kernel compares with, or None without a window."""
        if self.match_window is None:
            return None
        if span is None:
            span = self._pair_span if self._pair_span is not None else self.skipped_frames + 1
        return tuple(float(np.float32(r * span)) for r in self.match_window)

    def _pose_params(self):
        """What a pose step begun ahead must have been begun with to be this odometer's step (part of its ticket's key).  With a
        match window its effective radii are the last entry: a step begun with another window (another span) is never reused."""
        if self.klt_fused:
            Q = self.stereo.Q
            return ("klt", (float(Q[2, 3]), float(Q[2, 3]), float(-Q[0, 3]), float(-Q[1, 3])), int(self.pnp_iters), float(self.pnp_threshold),
                    int(self.pnp_seed), int(self.pnp_refine), int(self.pnp_lo_rounds), KltTrack(self.klt_window, self.klt_levels, self.klt_fb))
        tail = () if self.match_window is None else (self._window(),)
        if self.loop_check is not None:
            tail += (LoopCheck(self.loop_check),)
        if self.pose_method == "pnp":
            Q = self.stereo.Q
            if self.pnp_lo_rounds > 0:
                tail += (LoRounds(self.pnp_lo_rounds),)
            return ("pnp", float(self.match_threshold), (float(Q[2, 3]), float(Q[2, 3]), float(-Q[0, 3]), float(-Q[1, 3])),
                    int(self.pnp_iters), float(self.pnp_threshold), int(self.pnp_seed), int(self.pnp_refine), bool(self.cross_check)) + tail
        return (float(self.match_threshold), int(self.min_matches), float(max(self.rigidity_threshold, 0)),
                float(max(self.outlier_threshold, 0)), bool(self.cross_check)) + tail

    def _fused_ok(self):
        return (type(self) is StereoOdometer and type(self.matcher) is BFMatcher
                and (self.pose_method == "umeyama" or self._pnp_fused_ok())
                and not any(n in self.__dict__ for n in self._SEAMS))

    @staticmethod
    def _pnp_kwargs(params):
        """_pose_params() of the PnP mode as the keyword arguments of Context.pnp_pair / pnp_pair_begin (with a match window: of
        pnp_pair_window / pnp_pair_begin_window; with the LoRounds marker: of pnp_pair_lo / pnp_pair_begin_lo, which take the
        window and the loop check as keywords -- "lo_rounds" in the result says so)"""
        _, ratio, K4, iters, thr, seed, refine, cross_check = params[:8]
        kw = dict(ratio=ratio, K4=K4, iters=iters, thr=thr, seed=seed, refine=refine, want_matches=False, cross_check=cross_check)
        if isinstance(params[-1], LoRounds):
            kw["lo_rounds"], params = params[-1].rounds, params[:-1]
        params, loop = StereoOdometer._split_loop(params)
        if len(params) > 8:
            kw["window"] = params[8]
        if loop:
            kw.setdefault("window", None)       # (the loop check travels through the _window forms, with or without a window)
            kw.update(loop)
        return kw

    @staticmethod
    def _split_loop(params):
        """_pose_params() -> (the parameters without the loop entry, {} or {"loop": threshold})"""
        if params and isinstance(params[-1], LoopCheck):
            return params[:-1], {"loop": params[-1].max_hamming}
        return params, {}

    @staticmethod
    def _klt_kwargs(params):
        """_pose_params() of the fused Lucas-Kanade mode as the keyword arguments of Context.klt_pnp_pair / klt_pnp_pair_begin"""
        _, K4, iters, thr, seed, refine, lo_rounds, trk = params
        return dict(K4=K4, iters=iters, thr=thr, seed=seed, refine=refine, lo_rounds=lo_rounds, win=trk.win, levels=trk.levels, fb=trk.fb)

    def _step_begin(self, slot_a, slot_b, params):
        if params[0] == "klt":
            return self._ctx.klt_pnp_pair_begin(slot_a, slot_b, **self._klt_kwargs(params))
        if params[0] == "pnp":
            kw = self._pnp_kwargs(params)
            if "lo_rounds" in kw:
                return self._ctx.pnp_pair_begin_lo(slot_a, slot_b, **kw)
            return (self._ctx.pnp_pair_begin_window if "window" in kw else self._ctx.pnp_pair_begin)(slot_a, slot_b, **kw)
        params, loop = self._split_loop(params)
        return self._ctx.pose_pair_begin(slot_a, slot_b, *params, **loop)

    def _step_end(self, params, ticket):
        """Collect a step begun ahead with the _end of its kind."""
        if params[0] == "klt":
            return self._ctx.klt_pnp_pair_end(ticket)
        if params[0] == "pnp":
            if isinstance(params[-1], LoRounds):
                return self._ctx.pnp_pair_end_lo(ticket)
            return self._ctx.pnp_pair_end(ticket)
        return self._ctx.pose_pair_end(ticket)

    def _drop_specs(self, keep=()):
        """Collect and discard pose steps begun ahead.  A step's own error (e.g. VO_E_SWEEP on a pair it read) is discarded with
        it: it belongs to a result nobody asked for, and that pair's own update() reports what is wrong with it."""
        for key in [k for k in self._specs if k not in keep]:
            try:
                self._step_end(key[2], self._specs[key])
            except _native.VoError:
                pass
            finally:
                del self._specs[key]

    def reset_lookahead(self):
        """Collect and drop the pose steps begun ahead of time and the camera's unconsumed look-ahead pairs (they are
        recomputed when asked for).  Not in the reference: lets a caller start a measurement, or hand the camera to another
        odometer, with nothing in flight."""
        if self._ctx is not None:
            self._drop_specs()
        if hasattr(self.stereo, "reset_lookahead"):
            self.stereo.reset_lookahead()

    def _sparse_req(self):
        """the request of this odometer's sparse stereo chain, as StereoCamera.submit_sparse / SubmittedPair.sparse hold it"""
        from .stereo_camera import sparse_request
        return sparse_request(self.orb.nfeatures, self.MIN_VALID_DISPARITY, self.MAX_VALID_DISPARITY, self.sparse_row_tol, self.sparse_max_hamming,
                              self.sparse_mutual, self.sparse_ratio)

    def _start_next_pose(self):
        """The frame just accepted is the new `current`.  The pairs that will come next may already be on the device
        (look-ahead / submitted ahead): for as many of them as have FINISHED their disparity and keypoints (never waiting for
        one), start the matching + pose step now on a stream of its own -- (current, next), and, expecting every frame to be
        accepted, (next, next+1), ... up to `pose_ahead` steps.  In the steady state that is the next pair or none; when
        results arrive in a burst (a cold start: every pair in flight finishes at about the same time) the short kernel
        chains of many pairs run side by side instead of one after the other behind the host.  Purely an ordering change:
        _pair_fused looks a step up by its slots and parameters and computes on the spot when the guess was wrong."""
        if self.track == "map":        # (the map step needs the pose of the frame before it: nothing to begin ahead)
            return
        if self.match == "klt" and not self.klt_fused:      # (the composed tracking step is synchronous: nothing is begun ahead)
            return
        sparse = self.depth == "sparse"
        if not (self._klt_fused_ok() if self.match == "klt" else self._fused_ok()) or (not sparse and self.orb.last_slot_args is None):
            return self._drop_specs()
        # what identifies the keypoints a pair begun ahead will hold: the ORB arguments, or the sparse request (collected by the
        # waiting form of sparse_stereo: the slot is ready, so it only reads the slot's record)
        req = ("sparse",) + self._sparse_req() if sparse else self.orb.last_slot_args
        kps = self.current_kps
        if not self._on_device(kps, self.current_desc, self.current_3d):
            return self._drop_specs()
        depth = self.pose_ahead
        if sparse:      # (only pairs submitted under this very request: another one would be recomputed, which is update()'s business)
            nxt = [h.slot if h.sparse == req[1:] else None for h in self._next_hint]
        else:
            nxt = [h.slot for h in self._next_hint] if self._next_hint else self.stereo.next_lookahead_slots(depth)
        chain, counts = [kps.frame.slot], [len(kps)]
        for s in nxt[:depth]:
            if s is None or not self._ctx.slot_ready(s):
                break
            chain.append(s)
            key = (self.stereo.slot_key(s), req)
            if key not in self._ahead_counts:
                if len(self._ahead_counts) > 64:
                    self._ahead_counts.clear()
                try:
                    if sparse:
                        self.stereo._sparse_assoc(req[1:])
                        self._ahead_counts[key] = int(self._ctx.sparse_stereo(s, *req[1:6])[2])            # (finished: only collects the kept count)
                    else:
                        self._ahead_counts[key] = self._ctx.orb_slot_count(s, *self.orb.last_slot_args)   # (finished: only collects the count)
                except _native.VoError:
                    self._ahead_counts[key] = -1     # that pair's own update() reports what is wrong with it; nothing is begun on it here
            counts.append(self._ahead_counts[key])
        params = self._pose_params()
        sk = self.stereo.slot_key       # slot + generation: a slot refilled with another pair never matches
        wanted = []
        for j in range(len(chain) - 1):
            if not (0 < counts[j] <= 3800 and counts[j + 1] >= max(2, self.min_matches)):
                break                    # (a frame that will be rejected: what lies behind it pairs with another reference)
            wanted.append((sk(chain[j]), sk(chain[j + 1]), params))
        self._drop_specs(keep=wanted)
        from ._native import VoError
        for key in wanted:
            if key not in self._specs and len(self._specs) < _native.VO_NUM_POSE_ASYNC:
                try:
                    self._specs[key] = self._step_begin(key[0][0], key[1][0], params)
                except VoError:
                    break                    # nothing started: update() computes the step when it gets there

    def run(self, pairs, depth=None, on_sweep_timeout="raise"):
        """Feed an iterable of host (left, right) pairs through update(), keeping up to `depth` pairs
        submitted ahead so their upload and disparity overlap the tracking of the current pair.  Yields
        update()'s result per pair, in order.  Not in the reference (whose update() takes one host pair per call,
        stereo_odometer.py:115-116).

        The copy of each pair into pinned staging memory runs on the library's own staging thread (vo_host_stage_begin), one
        pair ahead of the pair being submitted: it overlaps this thread's kernel launches and waits, this thread never touches
        image bytes, and no second Python thread competes for the interpreter lock.  The caller may refill the arrays it
        yielded as soon as it is asked for the next pair (a copy is waited for before the iterator is advanced).  Pairs whose
        two images differ in channel count go through StereoCamera.submit() instead.  With depth="sparse" the pairs are submitted
        with this odometer's sparse request (StereoCamera.submit_staged(..., sparse=) / submit_sparse()): upload, both extractions,
        association and compaction run ahead on the look-ahead engines, update() collects, and pose steps are begun ahead on
        the pairs that have finished -- the results are those of update() pair by pair.

        A pair whose disparity is undefined (update() raises SweepTimeout, see there): with on_sweep_timeout="raise" (default)
        the exception leaves the generator, which ends -- the failed pair and the pairs already taken from `pairs` but not yet
        yielded (at most depth + 2) are lost to this run, every frame slot they held is given back, the odometer's state is
        that of the last yielded result, and a new run() may follow at once; with "skip" the generator yields None for that
        pair (neither accepted nor counted as skipped: the odometer's state is untouched) and carries on with the next one.
        Either way no slot stays reserved when the generator ends, however it ends (exhausted, closed, or by an exception)."""
        from collections import deque
        if on_sweep_timeout not in ("raise", "skip"):
            raise ValueError("on_sweep_timeout must be 'raise' or 'skip'")
        sparse = self._sparse_req() if self.depth == "sparse" else None     # (sparse pairs: no sweep group, so nothing to flush)
        cam, ctx = self.stereo, self.stereo._ctx
        depth = int(cam.lookahead if depth is None else depth)
        nbuf = _native.VO_NUM_HOST_STAGE
        it = iter(pairs)
        copying, queue = deque(), deque()            # staged (or being staged) and not yet submitted / submitted and not yet consumed
        state = {"k": 0, "done": False, "inflight": None}

        def stage_next():
            if state["inflight"] is not None:
                ctx.host_stage_wait(state["inflight"])                   # its source arrays are the caller's again
                state["inflight"] = None
            try:
                L, R = next(it)
            except StopIteration:
                state["done"] = True
                return
            L, R = np.asarray(L), np.asarray(R)
            if L.ndim != R.ndim or L.shape != R.shape:
                copying.append((None, L.copy(), R.copy()))               # mixed inputs: converted when submitted
            else:
                buf = state["k"] % nbuf
                copying.append((buf,) + ctx.host_stage_begin(buf, L, R))
                state["inflight"] = buf
                state["k"] += 1

        def keep_one_ahead():
            while not state["done"] and len(copying) < 2:
                stage_next()

        try:
            while True:
                keep_one_ahead()
                started = 0
                while len(queue) <= depth and copying and (len(copying) >= 2 or state["done"]):
                    started += 1
                    item = copying.popleft()
                    if item[0] is None and sparse is not None:
                        queue.append(cam.submit_request(item[1], item[2], sparse, self.preprocessed_frames))
                    elif item[0] is None:
                        queue.append(cam.submit(item[1], item[2], preprocessed=self.preprocessed_frames))
                    else:
                        buf, w, h, ch, _keep = item
                        if state["inflight"] == buf:
                            state["inflight"] = None                     # (submit_staged waits for the copy)
                        if sparse is not None:
                            queue.append(cam.submit_staged(buf, w, h, ch, self.preprocessed_frames, sparse=sparse))
                        else:
                            queue.append(cam.submit_staged(buf, w, h, ch, self.preprocessed_frames))
                    keep_one_ahead()
                # (see StereoCamera.compute_3d: after a burst or at the end of the input nothing follows that a held-back pair
                # could share its sweep launch with)
                if sparse is None and (started > 1 or (started and state["done"] and not copying)):
                    flush = getattr(ctx, "lookahead_flush", None)
                    if flush is not None:
                        flush()
                if not queue:
                    return
                head = queue.popleft()
                self._next_hint = tuple(queue)[:self.pose_ahead]
                try:
                    try:
                        res = self.update(head, None)
                    except _native.SweepTimeout:
                        if on_sweep_timeout != "skip":
                            raise
                        res = None
                    yield res
                finally:
                    self._next_hint = ()
        finally:
            if state["inflight"] is not None:                            # a copy begun and never submitted: its sources may go away now
                ctx.host_stage_wait(state["inflight"])
            # pairs submitted ahead that nobody will consume (the generator was closed early, or an exception ended it): their
            # slots are marked reserved and only a consumer ever un-marks one -- give them back, or up to depth + 1 of the 28
            # slots stay stranded and later submissions fall back to synchronous processing.  Pose steps begun ahead on them
            # are collected first (they read the slots); whatever still runs is ordered before a slot's next use.
            if any(sp.slot is not None for sp in queue):
                try:
                    self._drop_specs()
                finally:
                    for sp in queue:
                        cam.release_submitted(sp)
                    queue.clear()

    _SEAMS = ("point_clouds", "point_cloud_transform", "rigid_body_filter", "bilinear_interpolate_pixels",
              "_estimate", "_gate")

    def _try_pair(self, kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b, span=None):
        """span: the frames between a and b (None: skipped_frames + 1); it scales the match window."""
        self._pair_span = span
        try:
            return self._try_pair_span(kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b)
        finally:
            self._pair_span = None

    def _try_pair_span(self, kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b):
        if self.direct_refine or self.patch_refine:     # (the two exclude each other) the slots of the pair being tried, for the alignment
            on_dev = self._on_device(kps_a, desc_a, im3d_a) and self._on_device(kps_b, desc_b, im3d_b)
            pair = (kps_a.frame.slot, kps_b.frame.slot) if on_dev else None
            if self.direct_refine:
                self._direct_pair = pair
            else:
                self._patch_pair = pair
        if self.match == "klt":
            return self._pair_klt(kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b)
        # fused device path when nothing along the way was replaced by the user
        fused = (type(self) is StereoOdometer and type(self.matcher) is BFMatcher and 2 <= len(kps_b) and len(kps_a) <= 3800
                 and self._on_device(kps_a, desc_a, im3d_a) and self._on_device(kps_b, desc_b, im3d_b)
                 and not any(n in self.__dict__ for n in self._SEAMS))
        if self.pose_method == "pnp":
            if fused and self._pnp_fused_ok():
                return self._pair_pnp_fused(kps_a.frame.slot, kps_b.frame.slot)
            return self._pair_pnp(kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b)
        if fused:
            return self._pair_fused(kps_a.frame.slot, kps_b.frame.slot)
        pts_a, pts_b = self.point_clouds(kps_a, kps_b, desc_a, desc_b, im3d_a, im3d_b)
        if pts_a is None:
            self.skip_cause = "matches"
            return None
        return self.point_cloud_transform(pts_a, pts_b)

    def _pair_pnp(self, kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b):
        """Extension: pose of the pair by RANSAC solvePnP (3-D of frame a, pixels of frame b)."""
        if not (self._on_device(kps_a, desc_a, im3d_a) and self._on_device(kps_b, desc_b, im3d_b) and len(kps_b) >= 2):
            raise ValueError("pose_method='pnp' needs the device-resident frames compute_3d returns")
        q, t, pts_a, _, st_a, _ = self._ctx.point_clouds(kps_a.frame.slot, kps_b.frame.slot, self.match_threshold, self.cross_check,
                                                         **self._window_kw(), **self._loop_kw())
        if len(q) < self.min_matches:
            self.skip_cause = "matches"
            return None
        if (st_a == 2).any():
            raise ZeroDivisionError("division by zero")
        ok = (st_a == 0) & np.isfinite(pts_a).all(axis=1)
        x0, y0 = kps_b.frame.roi[0], kps_b.frame.roi[1]
        uv = kps_b.xy[t[ok]] + np.array([x0, y0], np.float32)      # keypoints live in the cropped image
        Q = self.stereo.Q
        K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
        if ok.sum() < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        r = self._ctx.ransac_pnp(pts_a[ok], uv, K4, self.pnp_iters, self.pnp_threshold, self.pnp_seed)
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None
        return self._gate(np.vstack([r["Rt"], [0, 0, 0, 1]]))

    def _pair_klt(self, kps_a, desc_a, im3d_a, kps_b, desc_b, im3d_b):
        """Extension (match="klt"): frame a's keypoints tracked into frame b (vo_klt_track), then the pose from (3-D of a, pixels
        of b) by RANSAC PnP with the decisions of _pair_pnp, or from (3-D of a, 3-D of b at the tracked positions) through
        point_cloud_transform.  A track is dropped, never an error, where a lookup has no usable tap or no finite point."""
        if not (self._on_device(kps_a, desc_a, im3d_a) and self._on_device(kps_b, desc_b, im3d_b)):
            raise ValueError("match='klt' needs the device-resident frames compute_3d returns")
        fa, fb = kps_a.frame, kps_b.frame
        if self.klt_fused and len(kps_a) <= 3800 and self._klt_fused_ok():
            return self._pair_klt_fused(fa.slot, fb.slot, len(kps_a))
        xy_b, st, _ = self._ctx.klt_track(fa.slot, fb.slot, win=self.klt_window, levels=self.klt_levels, fb=self.klt_fb)
        idx = np.nonzero(st == 0)[0]
        self.klt_counts = (len(st), len(idx))
        if len(idx) < self.min_matches:
            self.skip_cause = "matches"
            return None
        if self.depth == "sparse":
            pts_a = np.asarray(im3d_a, np.float32).reshape(-1, 3)[idx]           # the per-keypoint cloud
            ok = np.isfinite(pts_a).all(axis=1)
        else:
            pts_a, st_a = self._ctx.points3d_at(fa.slot, kps_a.xy[idx])
            ok = (st_a == 0) & np.isfinite(pts_a).all(axis=1)
        idx, pts_a = idx[ok], pts_a[ok]
        uv = xy_b[idx]
        if self.pose_method == "pnp":
            if len(idx) < max(self.min_matches, 4):
                self.skip_cause = "matches"
                return None
            Q = self.stereo.Q
            K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
            r = self._ctx.ransac_pnp(pts_a, uv + np.array([fb.roi[0], fb.roi[1]], np.float32), K4, self.pnp_iters, self.pnp_threshold, self.pnp_seed)
            if r["best_count"] < self.min_matches:
                self.skip_cause = "outlier"
                return None
            return self._gate(np.vstack([r["Rt"], [0, 0, 0, 1]]))
        # 3-D of frame b where the tracks ended: inside the crop only (a track may leave it and stay inside the image)
        cw, ch = fb.roi[2] - fb.roi[0], fb.roi[3] - fb.roi[1]
        inside = (uv[:, 0] >= 0) & (uv[:, 1] >= 0) & (uv[:, 0] < np.float32(cw)) & (uv[:, 1] < np.float32(ch))
        pts_a, uv = pts_a[inside], uv[inside]
        pts_b, st_b = self._ctx.points3d_at(fb.slot, uv)
        ok = (st_b == 0) & np.isfinite(pts_b).all(axis=1)
        pts_a, pts_b = pts_a[ok], pts_b[ok]
        if len(pts_a) < self.min_matches:
            self.skip_cause = "matches"
            return None
        return self.point_cloud_transform(pts_a, pts_b)

    def _pair_klt_fused(self, slot_a, slot_b, n_kp):
        """The PnP arm of _pair_klt in one native call (vo_klt_pnp_pair: one device synchronisation, nothing but the record comes
        back): the same decisions in the same order.  A lookup without a usable tap drops its track (flag bit 0 never raises); with
        pnp_refine > 0 the gates see the refined pose when the refinement succeeded."""
        params = self._pose_params()
        ticket = self._specs.pop((self.stereo.slot_key(slot_a), self.stereo.slot_key(slot_b), params), None)
        if ticket is not None:
            r = self._step_end(params, ticket)                           # started by an earlier update()
            self.klt_ahead += 1
        else:
            r = self._ctx.klt_pnp_pair(slot_a, slot_b, **self._klt_kwargs(params))
        if self.pnp_lo_rounds > 0:
            self.pnp_lo_counts = (r["lo_rounds"], r["lo_support"])
        self.klt_counts = (n_kp, r["matches"])
        if r["matches"] < self.min_matches:
            self.skip_cause = "matches"
            return None
        if r["n"] < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None
        Rt = r["Rt_refined"] if r["refine_status"] == 0 else r["Rt"]
        return self._gate(np.vstack([Rt, [0, 0, 0, 1]]))

    def _pair_pnp_fused(self, slot_a, slot_b, want_matches=False, record=None):
        """_pair_pnp in one native call (vo_pnp_pair: one device synchronisation, nothing but the record comes back): the same
        decisions in the same order; with pnp_refine > 0 the gates see the refined pose when the refinement succeeded.
        want_matches / record (the map step): the step delivers q / t / mask too and the whole record is left in record["r"]."""
        params = self._pose_params()
        ticket = None if want_matches else self._specs.pop((self.stereo.slot_key(slot_a), self.stereo.slot_key(slot_b), params), None)
        if ticket is not None:
            r = self._step_end(params, ticket)                           # started by an earlier update()
        else:
            kw = self._pnp_kwargs(params)
            if want_matches:
                kw["want_matches"] = True
            if "lo_rounds" in kw:
                r = self._ctx.pnp_pair_lo(slot_a, slot_b, **kw)
            else:
                r = (self._ctx.pnp_pair_window if "window" in kw else self._ctx.pnp_pair)(slot_a, slot_b, **kw)
        if "lo_rounds" in r:
            self.pnp_lo_counts = (r["lo_rounds"], r["lo_support"])
        if record is not None:
            record["r"] = r
        if r["matches"] < self.min_matches:
            self.skip_cause = "matches"
            return None
        if r["flags"] & 1:
            raise ZeroDivisionError("division by zero")
        if r["n"] < max(self.min_matches, 4):
            self.skip_cause = "matches"
            return None
        if r["best_count"] < self.min_matches:
            self.skip_cause = "outlier"
            return None
        Rt = r["Rt_refined"] if r["refine_status"] == 0 else r["Rt"]
        return self._gate(np.vstack([Rt, [0, 0, 0, 1]]))

    def _pair_fused(self, slot_a, slot_b):
        """point_clouds + point_cloud_transform in one native call (one device synchronisation);
        same decisions and skip_cause strings as the two methods."""
        from ._native import VoError
        params = self._pose_params()
        ticket = self._specs.pop((self.stereo.slot_key(slot_a), self.stereo.slot_key(slot_b), params), None)
        if ticket is not None:
            counts, rc, _, T34 = self._ctx.pose_pair_end(ticket)         # started by an earlier update()
        else:
            plain, loop = self._split_loop(params)
            counts, rc, _, T34 = self._ctx.pose_pair(slot_a, slot_b, *plain, **loop)
        M, n1, n2, flags = (int(v) for v in counts)
        if M < self.min_matches:
            self.skip_cause = "matches"
            return None
        if flags & 1:
            raise ZeroDivisionError("division by zero")
        too_few_rigid = n1 < 10
        if too_few_rigid:
            self.skip_cause = "rigidity"
        if rc[0] < 0:
            raise VoError(-5, "Points cannot be colinear" if rc[0] == -2 else "Umeyama needs at least 3 points")
        if n2 < self.min_matches:
            if not too_few_rigid:
                self.skip_cause = "outlier"
            return None
        if rc[1] < 0:
            raise VoError(-5, "Points cannot be colinear" if rc[1] == -2 else "Umeyama needs at least 3 points")
        return self._gate(np.vstack([T34, [0, 0, 0, 1]]))

    # ------------------------------------------------------------------------------------------
    def point_clouds(self, kps1, kps2, desc1, desc2, im3d1, im3d2):
        """Matched 3-D points of two frames (Mx3 float32 each) or (None, None)  [reference :162-175]."""
        fused = (type(self.matcher) is BFMatcher and self._on_device(kps1, desc1, im3d1)
                 and self._on_device(kps2, desc2, im3d2) and len(kps2) >= 2)
        if fused:
            q, t, pts1, pts2, st1, st2 = self._ctx.point_clouds(kps1.frame.slot, kps2.frame.slot,
                                                                self.match_threshold, self.cross_check, **self._window_kw(), **self._loop_kw())
            if len(q) < self.min_matches:
                return None, None
            if (st1 == 2).any() or (st2 == 2).any():
                raise ZeroDivisionError("division by zero")
            return pts1, pts2
        # generic path: the same steps through the public seams (any matcher / arrays)
        window = self._window()
        if window is None:
            knn = self.matcher.knnMatch
        else:
            if not hasattr(self.matcher, "knnMatchWindow"):
                raise ValueError("match_window needs a matcher with knnMatchWindow(query, train, queryKeypoints, trainKeypoints, window, k)")

            def knn(d1, d2, k):
                k1, k2 = (kps1, kps2) if d1 is desc1 else (kps2, kps1)
                return self.matcher.knnMatchWindow(d1, d2, k1, k2, window, k=k)
        matches = knn(desc1, desc2, k=2)
        if window is not None:
            matches = [m for m in matches if len(m) == 2]    # fewer than two candidates in the window: no ratio test, no match
        matches = [m[0] for m in matches if m[0].distance < self.match_threshold * m[1].distance]
        if self.cross_check:
            # a(j), the nearest query of every train descriptor: the matcher with the roles swapped (k = 1, ties -> lower index)
            back = knn(desc2, desc1, k=1)
            matches = [m for m in matches if len(back[m.trainIdx]) and back[m.trainIdx][0].trainIdx == m.queryIdx]
        if self.loop_check is not None:
            # the loop check: the right partners of the two matched keypoints must look alike too
            rd1, rd2 = getattr(im3d1, "right_desc", None), getattr(im3d2, "right_desc", None)
            if rd1 is None or rd2 is None:
                raise ValueError("loop_check needs the per-keypoint clouds compute_sparse returns (their right_desc)")
            rd1, rd2 = np.asarray(rd1, np.uint8).reshape(-1, 32), np.asarray(rd2, np.uint8).reshape(-1, 32)
            matches = [m for m in matches
                       if int(np.unpackbits(np.bitwise_xor(rd1[m.queryIdx], rd2[m.trainIdx])).sum()) <= self.loop_check]
        if len(matches) < self.min_matches:
            return None, None
        if self.depth == "sparse":
            # the clouds are per keypoint: indexed by the matches
            return (np.asarray(im3d1, np.float32)[[m.queryIdx for m in matches]], np.asarray(im3d2, np.float32)[[m.trainIdx for m in matches]])
        pts1 = [self.bilinear_interpolate_pixels(im3d1, *kps1[m.queryIdx].pt) for m in matches]
        pts2 = [self.bilinear_interpolate_pixels(im3d2, *kps2[m.trainIdx].pt) for m in matches]
        return np.array(pts1), np.array(pts2)

    def _window_kw(self):
        """the window of the pair being tried as the keyword of the context's calls (none without a window: a replaced
        point_clouds keeps the signature it has)"""
        w = self._window()
        return {} if w is None else {"window": w}

    def _loop_kw(self):
        """the loop check as the keyword of the context's calls (none without it, like _window_kw)"""
        return {} if self.loop_check is None else {"loop": self.loop_check}

    @staticmethod
    def _on_device(kps, desc, im3d):
        return (isinstance(kps, KeyPointList) and kps.frame is not None and kps.frame.live
                and desc is kps.desc and isinstance(im3d, DeviceImage) and im3d.frame is kps.frame)

    def _estimate(self, src, dst):
        """cv2.estimateAffine3D(src, dst, force_rotation=True)[0] with the homogeneous row appended."""
        T34, _ = self._ctx.umeyama(src, dst, True)
        return np.vstack([T34, [0, 0, 0, 1]])

    def point_cloud_transform(self, current_pts, next_pts):
        """Rigid transform current -> next (4x4) or None with skip_cause set  [reference :177-223]."""
        if self.rigidity_threshold > 0:
            keep = self.rigid_body_filter(current_pts, next_pts) > 0
            current_pts, next_pts = current_pts[keep], next_pts[keep]
        too_few_rigid = len(current_pts) < 10
        if too_few_rigid:
            self.skip_cause = "rigidity"
        if self.outlier_threshold > 0 and not too_few_rigid:
            # single-pass outlier rejection on the relative residual of a first fit  [:188-197]
            T = self._estimate(current_pts, next_pts)
            h_next = np.hstack([next_pts, np.ones((len(next_pts), 1))]).astype(np.float64)
            h_cur = np.hstack([current_pts, np.ones((len(current_pts), 1))]).astype(np.float64)
            errors = np.linalg.norm(h_next - h_cur @ T.T, axis=1) / np.linalg.norm(h_next, axis=1)
            keep = errors < self.outlier_threshold + np.median(errors)
            current_pts, next_pts = current_pts[keep], next_pts[keep]
        if len(current_pts) < self.min_matches:
            if not too_few_rigid:
                self.skip_cause = "outlier"
            return None
        return self._gate(self._estimate(current_pts, next_pts))

    def _gate(self, T):
        """NaN check and the motion gates of the reference [:207-223]."""
        if np.isnan(T).any():
            self.skip_cause = "nan"
            return None
        if self.direct_refine:
            T = self._direct(T)
        if self.patch_refine:
            T = self._patch(T)
        scale = self.skipped_frames + 1
        dist = np.linalg.norm(T[0:3, 3])
        angle = np.linalg.norm(self._ctx.rodrigues(T[0:3, 0:3]))
        too_far = dist > self.MAX_DISTANCE_CHANGE * scale
        too_turned = angle > self.MAX_ROTATION_CHANGE * scale
        if too_far:
            self.skip_cause = "bigdist"
        if too_turned:
            self.skip_cause = "bigrot"
        if too_far or too_turned:
            if self.direct_refine or self.patch_refine:
                self.pose_information = None            # (the pose it belongs to was refused)
            return None
        return T

    def _guarded(self, T, Tr, guard):
        """whether the refined pose Tr lies within guard = (metres, radians) x (skipped_frames + 1) of the feature pose T"""
        D = Tr @ np.linalg.inv(T)                       # what the alignment moved the pose by
        scale = self.skipped_frames + 1
        dist = np.linalg.norm(D[0:3, 3])
        angle = np.arccos(min(1.0, max(-1.0, (np.trace(D[0:3, 0:3]) - 1.0) / 2.0)))
        return not (dist > guard[0] * scale or angle > guard[1] * scale)

    def _patch(self, T):
        """patch_refine: the feature pose T (4 x 4, a -> b) of the pair being tried -> the pose the gates see: the patch alignment's
        where it ended with status 0 and within patch_guard of T, T itself otherwise (_direct's rule)."""
        if self._patch_pair is None:
            raise ValueError("patch_refine=True needs the device-resident frames compute_sparse returns")
        Q = self.stereo.Q
        K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
        r = self._ctx.direct_align_kp(self._patch_pair[0], self._patch_pair[1], K4, T[:3], levels=self.patch_levels, iters=self.patch_iters,
                                      patch=self.patch_size)
        self.patch_status, self.patch_record, self.patch_accepted = r["status"], r, False
        self.pose_information = None                    # (of the pose this step delivers, never of an older one)
        if r["status"] != 0 or not np.isfinite(r["Rt"]).all():
            return T
        Tr = np.vstack([r["Rt"], [0, 0, 0, 1]])
        if not self._guarded(T, Tr, self.patch_guard):
            return T
        self.patch_accepted = True
        self.pose_information = r["information"]
        return Tr

    def _direct(self, T):
        """direct_refine: the feature pose T (4 x 4, a -> b) of the pair being tried -> the pose the gates see: the dense direct
        alignment's where it ended with status 0 and within direct_guard of T, T itself otherwise."""
        if self._direct_pair is None:
            raise ValueError("direct_refine=True needs the device-resident frames compute_3d returns")
        Q = self.stereo.Q
        K4 = [Q[2, 3], Q[2, 3], -Q[0, 3], -Q[1, 3]]
        r = self._ctx.direct_align(self._direct_pair[0], self._direct_pair[1], K4, T[:3], levels=self.direct_levels, iters=self.direct_iters,
                                   max_points=self.direct_max_points, dmin=self.MIN_VALID_DISPARITY, dmax=self.MAX_VALID_DISPARITY,
                                   **(dict(affine=True) if self.direct_affine else {}))
        self.direct_status, self.direct_record, self.direct_accepted = r["status"], r, False
        if self.direct_affine:                          # (an estimate exists once a free iteration completed: the third is the first)
            self.direct_brightness = (r["gain"], r["offset"]) if r["iters_done"] >= 3 else None
        self.pose_information = None                    # (of the pose this step delivers, never of an older one)
        if r["status"] != 0 or not np.isfinite(r["Rt"]).all():
            return T
        Tr = np.vstack([r["Rt"], [0, 0, 0, 1]])
        if not self._guarded(T, Tr, self.direct_guard):
            return T
        self.direct_accepted = True
        self.pose_information = r["information"]
        return Tr

    def current_pose(self):
        """Camera pose in world (= first accepted frame) coordinates  [reference :225-226]."""
        return np.linalg.inv(self.c_T_w)
