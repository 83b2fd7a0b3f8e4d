/*
 * vo355.h -- C ABI of libvo355.so: the MI355X (gfx950) implementation of openVO's
 * stereo-odometry hot path.  Plain pointers and sizes only; no torch / C++ types.
 *
 * The reference (KevinSpevak/openVO) has no FFI of its own: its boundary is the set of
 * cv2 object call sites inside StereoCamera.compute_3d and StereoOdometer.update.  Each
 * entry point below names the reference line(s) it replaces (paths relative to
 * /root/reference/src/openVO/).  The Python classes in openvo_amd/ bind these with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success, a negative VO_E_* code otherwise;
 * vo_last_error(ctx) returns a message owned by the context.  Host pointers are
 * caller-owned, C-contiguous, and never retained past the call.  Device memory belongs to
 * the opaque context.  A context is bound to one device and one HIP stream and is NOT
 * thread-safe; use one context per thread / per GPU.  No C++ exception crosses the ABI.
 * There is no CPU fallback: if no gfx950 device is usable, vo_create fails.
 */
#ifndef VO355_H
#define VO355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vo_ctx vo_ctx;

enum {
    VO_OK = 0,
    VO_E_ARG = -1,     /* bad argument / shape */
    VO_E_HIP = -2,     /* HIP runtime error (message has the hipError string) */
    VO_E_STATE = -3,   /* call order violated (e.g. no disparity in that slot yet) */
    VO_E_CAP = -4,     /* capacity given at vo_create exceeded */
    VO_E_NUMERIC = -5, /* degenerate input (Umeyama: <3 points / colinear) */
    VO_E_SWEEP = -6    /* the disparity a result depends on is undefined: a strip hand-off inside the aggregation sweep of that
                          pair gave up waiting (an oversubscribed GPU).  Nothing computed from it is handed out; the pair can be
                          submitted again.  cv2's StereoSGBM is one sequential pass and cannot fail this way (stereo_camera.py:51) */
};

#define VO_NUM_SLOTS 28 /* frame slots per context: the odometer keeps prev and current, up to 25 more hold
                           look-ahead pairs (vo_prefetch_*), one is spare */

/* lifetime ------------------------------------------------------------------------- */
int vo_create(int device_id, int max_w, int max_h, int max_disp, int max_kp, vo_ctx** out);
void vo_destroy(vo_ctx* ctx);
const char* vo_last_error(const vo_ctx* ctx);
int vo_device_name(const vo_ctx* ctx, char* buf, int buflen);
int vo_synchronize(vo_ctx* ctx);
/* How many look-ahead engines the context may use (each owns a HIP stream and a full SGBM + ORB workspace, allocated on its
 * first use: ~0.95 GB at 1280x720 / D = 128).  n <= 0 only asks.  Returns the count in effect (clamped to 1 .. 24 and to what
 * fits 40 % of the device's free memory), or a negative status.  May be called at any time; engines already created above a
 * lowered count keep their memory until vo_destroy but receive no further pairs.  The reference has no counterpart (cv2 keeps
 * one StereoSGBM object per StereoCamera, stereo_camera.py:23): this bounds the footprint of the replacement.
 * While sweep groups are in force (below) the dense look-ahead pairs of all engines travel on the context's two lane streams:
 * an engine then contributes its workspaces and staging, not its stream, and the automatic group size follows the count
 * (half the engines, so that consecutive groups use disjoint engines).  The open group is closed by a change of the count. */
int vo_set_engines(vo_ctx* ctx, int n);

/* one-off configuration (stereo_camera.py:16-27) ------------------------------------ */
/* map_left_1/2, map_right_1/2 of cv2.initUndistortRectifyMap(..., CV_16SC2)  [stereo_camera.py:19-22] */
int vo_set_rectify_maps(vo_ctx* ctx, int cam /*0=L,1=R*/, const int16_t* map1 /*h*w*2*/,
                        const uint16_t* map2 /*h*w*/, int w, int h);
/* cv2.StereoSGBM_create positional parameters [stereo_camera.py:23-27]; mode 0 = MODE_SGBM
 * (5 paths, the reference's default), 1 = MODE_HH (8 paths), 2 = MODE_SGBM_3WAY (3 paths; the reference's
 * "# TODO: mode option", stereo_camera.py:26); any other value is VO_E_ARG (MODE_HH4 = 3 included) and leaves the
 * parameters in force untouched.
 * Mode 2 is MODE_SGBM with the direction set W, E, N in place of W, NW, N, NE, E, and nothing else changed: the cost
 * volume (C carries + P2); L_r by Hirschmueller's eq. 13 with the zero vector as the predecessor outside the computed band;
 * S = min(L_W + L_E + L_N, 32767); the first minimum, the uniqueness test and "every sum saturated = no winner"; the disp2
 * arbitration, the sub-pixel step and the two-sided left-right check; medianBlur(3) and the speckle filter.  The N path runs
 * from the top row of the image to the bottom row as ONE stripe.  Parity with OpenCV's computeDisparity3WAY is NOT claimed:
 * that function, as recalled, cuts the image into horizontal stripes by thread count and restarts the vertical path in
 * each, so its output depends on the machine; this definition does not.  Mode 2 runs on the look-ahead engines like
 * MODE_HH, each pair's chain on its engine's stream: it joins no sweep group. */
int vo_set_sgbm(vo_ctx* ctx, int minDisparity, int numDisparities, int blockSize, int P1, int P2,
                int disp12MaxDiff, int preFilterCap, int uniquenessRatio, int speckleWindowSize,
                int speckleRange, int mode);
/* The matching cost in front of the aggregation.  BT (Birchfield-Tomasi + SAD, OpenCV's) is what a fresh context has and the only
 * cost for which parity with OpenCV is claimed.  CENSUS is an extra with no OpenCV counterpart and no oracle; its yardstick is the
 * definition in tests/sgbm_census_def.py, which the device equals bit for bit:
 *   signature   of pixel (x, y) for a window census_w x census_h (3, 5, 7 or 9 wide, 3, 5 or 7 high: at most 62 comparisons): the
 *               set of offsets (dx, dy) != (0, 0), |dx| <= census_w / 2, |dy| <= census_h / 2, whose pixel is strictly darker,
 *               I(x + dx, y + dy) < I(x, y).  Coordinates outside the image are clamped (rows and columns replicated).  The order
 *               of the bits is unspecified: only the number of comparisons in which two signatures differ is observable.
 *   pixel cost  the Hamming distance of sig_L(x, y) and sig_R(x - d, y), at the left columns of the computed band
 *               [max(minD + D, 0), w + min(minD, 0)), where x - d never leaves the image
 *   block cost  C = P2 + the blockSize x blockSize box sum of the pixel cost, its indices clamped to the band and to the image rows
 *               exactly as with BT; blockSize 1 is the bare Hamming cost.  preFilterCap means nothing to this cost.
 * Everything behind C -- the paths of modes 0, 1 and 2, the winner stage, both post filters -- is unchanged.  A signature depends
 * only on the ORDER of the grey levels in its window, so any strictly increasing change of either image's intensities leaves the
 * disparity image bit-identical.  P1 / P2 want rescaling to the Hamming range (some 2 / 8 x blockSize^2 in place of 8 / 32).
 * The setting lives beside vo_set_sgbm's parameters and persists across vo_set_sgbm.  VO_E_ARG, the setting in force staying in
 * force: a cost other than 0 or 1; with cost 1 a window outside {3,5,7,9} x {3,5,7}.  With cost 0 the window arguments are
 * ignored.  A call that changes nothing does nothing; one that changes something first closes the open sweep group (pairs already
 * enqueued finish under the cost they began with).  A census pair runs on the look-ahead engines like a mode 2 pair, its chain on
 * its engine's stream: it joins no sweep group.  No overflow refusal is needed beyond vo_set_sgbm's: the largest census block cost
 * is 121 x 62 = 7502, below the smallest BT bound vo_set_sgbm already admits (at the smallest preFilterCap a BT pixel cost reaches 2 x 15 + 63 = 93 where a census one reaches 62). */
#define VO_SGBM_COST_BT      0   /* Birchfield-Tomasi + SAD, OpenCV's: the default */
#define VO_SGBM_COST_CENSUS  1
int vo_set_sgbm_cost(vo_ctx* ctx, int cost, int census_w, int census_h);
int vo_get_sgbm_cost(const vo_ctx* ctx, int* cost, int* census_w, int* census_h);   /* all three pointers are required */
/* C (block cost + P2, either cost) of the latest synchronous SGBM run (vo_sgbm_compute, vo_sgbm_compute_host, ...) in the main
 * workspace, as [H][W1][D] without the padding of d to a multiple of 32; W1 is the width of the computed band.  cells must equal
 * H * W1 * D (VO_E_ARG otherwise); VO_E_STATE when there is none (no run yet, an empty band, or a look-ahead pair has used the
 * workspace since).  A seam for tests: it pins the cost stage directly instead of through the winner stage. */
int vo_sgbm_cost_volume(vo_ctx* ctx, int16_t* out, size_t cells);
/* Q of cv2.stereoRectify [stereo_camera.py:17-18], row-major 4x4 */
int vo_set_Q(vo_ctx* ctx, const double* Q16);
/* slice bounds used by crop_to_valid_region_left [stereo_camera.py:35-37]:
 * rows y0:y1, cols x0:x1 where (x0,y0,x1,y1) = valid_region_left (quirk kept) */
int vo_set_roi(vo_ctx* ctx, int x0, int y0, int x1, int y1);

/* per frame pair (stereo_camera.py:43-55) -------------------------------------------- */
/* cvtColor(BGR2GRAY) if channels==3 [:44-47]; remap x2 unless preprocessed [:48-50].
 * Leaves rectified gray left/right on the device in `slot`. */
int vo_upload_pair(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h,
                   int channels, int preprocessed);
/* streaming ingest: keep n input pairs resident in HBM (vo_stage_pairs_alloc + vo_stage_pair),
 * then feed a slot from pair `index` without touching the host (same processing as vo_upload_pair) */
int vo_stage_pairs_alloc(vo_ctx* ctx, int n, int w, int h, int channels);
int vo_stage_pair(vo_ctx* ctx, int index, const uint8_t* left, const uint8_t* right);
int vo_load_staged_pair(vo_ctx* ctx, int slot, int index, int preprocessed);
/* look-ahead: ingest + StereoSGBM of staged pair `index` into `slot` on the context's second stream,
 * asynchronously; later calls that use the slot wait for it on the device.  Lets the next pair's
 * disparity overlap the current pair's ORB / matching / pose kernels. */
int vo_prefetch_staged_pair(vo_ctx* ctx, int slot, int index, int preprocessed);
/* look-ahead pairs submitted and not yet waited for or dropped (instrumentation; the reference is synchronous:
 * stereo_odometer.py:115-117 computes one pair per update() call) */
int vo_lookahead_depth(vo_ctx* ctx, int* depth_out);
/* the caller gives up a look-ahead slot without consuming it (a prediction of the next pair that did not come true) */
int vo_lookahead_drop(vo_ctx* ctx, int slot);
/* Sweep groups.  With a hardware queue per stream (GPU_MAX_HW_QUEUES >= engines + 4) every look-ahead pair's kernels are
 * enqueued when it is submitted.  With fewer queues the library collects up to B submitted pairs whose early stages are
 * enqueued and runs their aggregation sweeps as ONE launch; a pair's remaining work follows when its group closes: when it
 * has B members, when anything is about to wait on, read, refill or drop a member's slot (so no call ever sees a half-done
 * slot), or when the caller says that no further pair follows now (vo_lookahead_flush).  Results do not depend on B.
 * While B > 1 the dense look-ahead pairs go on two lane streams the context owns instead of the engines' own: a group's
 * members and its launches share one lane and consecutive groups alternate, so a group's early stages run beside the launches
 * of the group before it.  Without a request B follows the queue budget: 1 with a queue per stream, min(12, engines / 2) with
 * fewer.  VO_GROUP_LANES=0 in the environment at vo_create keeps every engine on its own stream (B without a request is then
 * min(12, engines)).  Sparse and monocular look-ahead submissions always use the engines' own streams.
 * On a lane the members also leave their planes and cost volumes to the group: F members' worth, or however many are pending when
 * the group closes, go in one launch each (F = 8 without a request).  Whatever would change what a pending launch still reads
 * -- vo_stage_pairs_alloc, vo_stage_pair, a setter, a consumer of a member's slot, vo_synchronize -- has them launched first,
 * with the parameters in force when each pair was submitted.  VO_GROUP_FRONTS=n in the environment at vo_create sets F; 0
 * gives every pair its own two launches, as without lanes.
 * vo_set_sweep_group: n <= 0 only asks, otherwise B = min(n, VO_MAX_SWEEP_GROUP) from now on (the open group is closed);
 * returns the size in force (never above the number of engines) or a negative status.  VO_SWEEP_GROUP in the environment
 * does the same at vo_create.  vo_lookahead_flush closes the open group and returns the size in force as well -- 1 tells a
 * caller that flushing never matters.  vo_sweep_group_stats: groups closed so far {full, by a consumer, by a flush, by a
 * change of parameters / engines / geometry} and the members of the open one (instrumentation).  The reference has no
 * counterpart (it computes one pair per call, stereo_odometer.py:115-117). */
#define VO_MAX_SWEEP_GROUP 12
int vo_set_sweep_group(vo_ctx* ctx, int n);
int vo_lookahead_flush(vo_ctx* ctx);
int vo_sweep_group_stats(vo_ctx* ctx, int64_t* closed4, int* open_members);
/* the same from host images -- the caller's decode/ingest step in front of update():
 * copied to pinned staging, uploaded asynchronously on the engine's stream, then as above.  The host
 * buffers are free again when the call returns. */
int vo_prefetch_pair(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h,
                     int channels, int preprocessed);
/* the same in two halves, so that the thread that launches kernels does no memcpy (the reference hands host arrays to
 * update(), stereo_odometer.py:115-116): vo_host_stage_pair copies the two images into pinned staging buffer `buf`
 * (0 .. VO_NUM_HOST_STAGE-1) -- it first waits until the previous upload out of that buffer has finished, and it is the ONE
 * entry point that may run on another thread while the context is in use (it touches nothing but that buffer; two calls
 * must not name the same buffer concurrently); vo_prefetch_host_staged then starts upload + SGBM (+ ORB) of that buffer's
 * pair on a look-ahead engine like vo_prefetch_pair.
 * vo_host_stage_begin hands the same copy to ONE staging thread owned by the library and returns at once (a host written in
 * an interpreted language then needs no thread of its own, and no interpreter lock changes hands per pair); the two images
 * must stay untouched until vo_host_stage_wait, vo_prefetch_host_staged or vo_host_stage_fetch on that buffer has returned
 * (each waits for the copy).  openvo_amd.StereoOdometer.run() keeps a few copies ahead of the pair it submits. */
#define VO_NUM_HOST_STAGE 20
int vo_host_stage_pair(vo_ctx* ctx, int buf, const uint8_t* left, const uint8_t* right, int w, int h, int channels);
int vo_host_stage_begin(vo_ctx* ctx, int buf, const uint8_t* left, const uint8_t* right, int w, int h, int channels);
int vo_host_stage_wait(vo_ctx* ctx, int buf);
int vo_prefetch_host_staged(vo_ctx* ctx, int slot, int buf, int w, int h, int channels, int preprocessed);
/* the pair staging buffer `buf` holds, copied back out (a caller that found no free slot keeps the pair on the host) */
int vo_host_stage_fetch(vo_ctx* ctx, int buf, uint8_t* left, uint8_t* right, int w, int h, int channels);
/* look-ahead keypoints: when enabled, every vo_prefetch_staged_pair also runs the ORB extraction
 * (same arguments as vo_orb_detect_and_compute) behind the SGBM on the engine's stream; a later
 * vo_orb_detect_and_compute on that slot with the SAME arguments only waits and downloads, any
 * other arguments recompute.  Results are identical either way. */
int vo_set_lookahead_orb(vo_ctx* ctx, int enable, int nfeatures, int mask_mode, int min_disp16, int max_disp16);
/* self.stereoSGBM.compute(L, R) [:51]: int16 disparity x16 of the slot's pair; kept on the
 * device; disp16_out (h*w) may be NULL */
int vo_sgbm_compute(vo_ctx* ctx, int slot, int16_t* disp16_out);
/* stand-alone stereoSGBM.compute on host images (the cv2 object seam) */
int vo_sgbm_compute_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h,
                         int16_t* disp16_out);
/* lazy materialisation of compute_3d's return values [:51-55], FULL (uncropped) images */
int vo_download_disparity_f32(vo_ctx* ctx, int slot, float* out /*h*w*/);
int vo_download_xyz(vo_ctx* ctx, int slot, float* out /*h*w*3*/); /* cv2.reprojectImageTo3D [:52] */
int vo_download_left(vo_ctx* ctx, int slot, uint8_t* out /*h*w*/);
int vo_download_right(vo_ctx* ctx, int slot, uint8_t* out /*h*w*/);
/* stand-alone helpers at the cv2 seams */
int vo_cvt_bgr2gray(vo_ctx* ctx, const uint8_t* bgr, int w, int h, uint8_t* gray);      /* [:45,47] */
int vo_remap(vo_ctx* ctx, int cam, const uint8_t* src, int w, int h, uint8_t* dst);     /* [:30,33] */
int vo_reproject_to_3d(vo_ctx* ctx, const float* disp, int w, int h, const double* Q16,
                       float* xyz /*h*w*3*/);                                           /* [:52] */

/* features (stereo_odometer.py:22,38-41,117) ------------------------------------------ */
/* orb.detectAndCompute(next_img, feature_mask(next_disp)) on the slot's cropped left image.
 * mask_mode 0: no mask; 1: feature_mask fused -- pixel allowed iff
 * min_disp16 <= disp16 <= max_disp16 (MIN/MAX_VALID_DISPARITY*16, [stereo_odometer.py:6-7,38-41]).
 * Results stay on the device in the slot; host outputs may each be NULL.  Keypoints come in
 * canonical order (octave, y, x).  *n_out may exceed nfeatures (OpenCV keeps response ties). */
int vo_orb_detect_and_compute(vo_ctx* ctx, int slot, int nfeatures, int mask_mode, int min_disp16,
                              int max_disp16, float* kp_xy /*cap*2*/, float* kp_size,
                              float* kp_angle, float* kp_response, int32_t* kp_octave,
                              uint8_t* desc /*cap*32*/, int cap, int* n_out);
/* the cv2 object seam on host arrays: img (h rows, stride bytes), mask NULL or same geometry */
int vo_orb_detect_and_compute_host(vo_ctx* ctx, const uint8_t* img, int w, int h, int stride,
                                   const uint8_t* mask, int mask_stride, int nfeatures,
                                   float* kp_xy, float* kp_size, float* kp_angle,
                                   float* kp_response, int32_t* kp_octave, uint8_t* desc, int cap,
                                   int* n_out);
int vo_slot_num_keypoints(vo_ctx* ctx, int slot, int* n_out);
/* download what vo_orb_detect_and_compute left in the slot (when that call passed NULL outputs to keep
 * everything on the device); any output may be NULL */
int vo_download_keypoints(vo_ctx* ctx, int slot, float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                          int32_t* kp_octave, uint8_t* desc, int cap, int* n_out);

/* matching (stereo_odometer.py:163-164) ------------------------------------------------ */
/* matcher.knnMatch(q, t, k=2) with NORM_HAMMING: idx/dist nq*2, ascending distance, ties ->
 * lower train index; -1 / INT32_MAX where the train set has fewer than 2 rows */
int vo_bf_knn2_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                       int32_t* idx, int32_t* dist);
/* Cross-check (mutual nearest neighbours), an EXTENSION of the matcher [stereo_odometer.py:21 "# TODO crosscheck", above
 * cv2.BFMatcher.create(cv2.NORM_HAMMING)]:
 *   b(i) = the nearest train of query i, ties -> lower train index (= idx[2 i] of vo_bf_knn2_hamming);
 *   a(j) = the nearest query of train j, ties -> lower query index;
 *   query i passes iff b(i) exists and a(b(i)) == i.
 * That is mutual nearest neighbour with OpenCV's tie rule in both directions, which is what OpenCV's
 * BFMatcher(NORM_HAMMING, crossCheck=true) / batchDistance(crosscheck=true) is believed to produce -- from memory of its code,
 * parity unpinned (no OpenCV to compare against where this was written; tests/test_crosscheck_host.py pins it wherever a cv2
 * is importable).  a(j) comes out of the SAME kernel launch as the kNN-2 (column minima of the distance tiles): the matcher
 * runs once, not twice.  Cross-check needs nq <= 65535 (VO_E_CAP otherwise).
 * match_flags of the _ex entries below: bit 0 = VO_MATCH_CROSSCHECK, bit 1 = VO_MATCH_WINDOW, bit 2 = VO_MATCH_LOOP (the stereo pair
 * steps only); every other bit must be 0.  The
 * entries without _ex are the same calls with match_flags = 0, unchanged.
 * Window (VO_MATCH_WINDOW), a second EXTENSION of the matcher [stereo_odometer.py:165 "# TODO config" at the match step]: train j
 * is a candidate of query i only if |xq_i - xt_j| <= rx and |yq_i - yt_j| <= ry, evaluated in float32 on the keypoint positions the
 * two slots hold (ROI-cropped pixels); a NaN coordinate is in no window.  idx / dist are the two lexicographically smallest
 * (distance, train index) AMONG THE CANDIDATES, {-1, INT32_MAX} where there are fewer than two -- a query with fewer than two
 * candidates gives no match in any consumer (the ratio test needs both).  With VO_MATCH_CROSSCHECK as well, a(j) is taken over the
 * queries that have j in their window (the test is symmetric): a match must be mutual within the window.  rx = ry = 0 is legal
 * (equal positions only); a window larger than the image gives the plain kernel's result bit for bit.  The same launch as the
 * plain kNN-2: the window is a mask on its keys, and tiles of 16 trains whose bounding box is out of reach of a wave's 64 queries
 * are skipped (keypoints are stored in (octave, y, x) order, so most are).
 * The radii are context state (vo_set_match_window), read when a step is ENQUEUED: a step begun ahead keeps the window it was
 * begun with.  VO_MATCH_WINDOW without a window set is VO_E_ARG.  The ratio test inside a window is laxer than over the whole
 * image (the runner-up is the best of fewer candidates). */
#define VO_MATCH_CROSSCHECK 1
#define VO_MATCH_WINDOW 2
/* Loop check (VO_MATCH_LOOP), a third EXTENSION, for the stereo pair steps on slots whose keypoints carry depth (vo_sparse_stereo):
 * a match (q, t) that has passed the ratio test -- and the cross-check and the window where asked for -- is kept iff the right-image
 * partners of q and t look alike too: popcount(kp_rdesc_a[q] ^ kp_rdesc_b[t]) <= max_hamming (the circular matching of sparse
 * stereo odometry; tests/sparse_loop_ref.py restates it).  M counts what passes every test and every later stage works on that
 * set; a threshold of 256 gives the step without the flag, bit for bit.  The threshold is context state like the window
 * (vo_set_match_loop, 0 .. 256), read when a step is ENQUEUED: a step begun ahead keeps the threshold it was begun with; it is not
 * scaled with the frames a pair spans.  VO_MATCH_LOOP without a threshold set is VO_E_ARG; on a slot whose keypoints carry no
 * depth it is VO_E_STATE; vo_point_clouds_ex, vo_pose_pair_ex / _begin_ex and vo_pnp_pair / _begin take it, every other entry
 * with match_flags (the monocular steps, the kNN seams) answers VO_E_ARG. */
#define VO_MATCH_LOOP 4
int vo_set_match_loop(vo_ctx* ctx, int max_hamming);
/* VO_E_STATE when no threshold is set */
int vo_clear_match_loop(vo_ctx* ctx);
/* finite radii >= 0 (VO_E_ARG otherwise: negative, NaN, inf) */
int vo_set_match_window(vo_ctx* ctx, float rx, float ry);
/* back to no window; VO_E_STATE when none is set (like every call made out of order) */
int vo_clear_match_window(vo_ctx* ctx);
/* the windowed kNN-2 on host arrays: xy_q / xy_t are nq / nt (x, y) float pairs, the radii are arguments (the context's window is
 * neither read nor changed); match_flags may add VO_MATCH_CROSSCHECK, and only then are mutual (nq bytes, required) and t_best
 * (nt x 2, may be NULL) written, as by vo_bf_knn2_hamming_mutual */
int vo_bf_knn2_hamming_window(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, const float* xy_q, const float* xy_t,
                              float rx, float ry, int match_flags, int32_t* idx, int32_t* dist, uint8_t* mutual, int32_t* t_best);
/* vo_bf_knn2_hamming's idx / dist of the same launch, plus mutual (nq bytes: 1 = query i passes the cross-check) and, when
 * t_best is not NULL, t_best (nt x 2 int32): {a(j), its distance}, {-1, INT32_MAX} when there is no query */
int vo_bf_knn2_hamming_mutual(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist,
                              uint8_t* mutual, int32_t* t_best);
/* m[0].distance < ratio * m[1].distance in double on float32 distances [:164]; host only */
int vo_ratio_filter(const int32_t* idx, const int32_t* dist, int nq, double ratio, int32_t* q_out,
                    int32_t* t_out, int* m_out);

/* 3-D lookup (stereo_camera.py:52 fused with stereo_odometer.py:50-79) ------------------ */
/* bilinear_interpolate_pixels of the slot's (cropped) reprojected image at float keypoint
 * coords; status 0 ok, 1 NaN, 2 no usable tap (reference raises ZeroDivisionError) */
int vo_points3d_at(vo_ctx* ctx, int slot, const float* xy, int n, float* xyz_out /*n*3*/,
                   uint8_t* status_out);
/* same on an explicit host H*W*3 float image (the reference method's own signature) */
int vo_bilinear_at(vo_ctx* ctx, const float* img3d, int w, int h, const float* xy, int n,
                   float* out, uint8_t* status_out);

/* fused pair step: point_clouds(kps_a, kps_b, desc_a, desc_b, 3d_a, 3d_b) [:162-175] entirely on
 * the device for two slots: kNN-2 + ratio + both 3-D lookups.  Returns M matches in match order
 * (ascending query index); outputs may be NULL except m_out. */
int vo_point_clouds(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int32_t* q_idx,
                    int32_t* t_idx, float* pts_a /*cap*3*/, float* pts_b, uint8_t* status_a,
                    uint8_t* status_b, int cap, int* m_out);
/* the same; with VO_MATCH_CROSSCHECK a match must pass the ratio test AND its m[0] the cross-check */
int vo_point_clouds_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, int32_t* q_idx,
                       int32_t* t_idx, float* pts_a, float* pts_b, uint8_t* status_a,
                       uint8_t* status_b, int cap, int* m_out);

/* fused pair step with ONE host synchronisation: point_clouds [:162-175] followed by the filtering
 * and fitting part of point_cloud_transform [:177-205] for two device-resident slots.
 * counts4 = {M matches after the ratio test, n1 after the rigid-body filter (= M when
 * rigidity_thr <= 0), n2 after the outlier pass (= n1 when it did not run), flags}; flags bit0: a
 * 3-D lookup had no usable tap (reference raises ZeroDivisionError), bit1: NaN residual.
 * rc2 = Umeyama status of {first fit, final fit}: 0 ok, 1 not attempted, -1 fewer than 3 points,
 * -2 "Points cannot be colinear".  T2_12 = final 3x4 transform (valid when rc2[1] == 0); T1_12 may be
 * NULL.  The caller applies the motion gates [:207-221]. */
int vo_pose_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int min_matches, double rigidity_thr,
                 double outlier_thr, int32_t* counts4, int32_t* rc2, double* T1_12, double* T2_12);
/* the same step split in two so that the host does not wait for it: _begin enqueues it on a stream of its
 * own (ordered behind the producers of both slots) and returns a ticket, _end waits for that ticket and
 * delivers what vo_pose_pair would have.  At most VO_NUM_POSE_ASYNC tickets may be open (each has scratch and a pinned record
 * of its own; they share three streams; tickets may end in any order).  Lets the pose steps of the pairs whose frames are already on the
 * device run while the caller still handles an earlier pair. */
#define VO_NUM_POSE_ASYNC 8
int vo_pose_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int min_matches, double rigidity_thr,
                       double outlier_thr, int* ticket_out);
int vo_pose_pair_end(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* rc2, double* T1_12, double* T2_12);
/* vo_pose_pair / vo_pose_pair_begin with match_flags (VO_MATCH_CROSSCHECK: as vo_point_clouds_ex; M counts the matches that
 * pass both tests, every later stage works on them).  A ticket's flags are part of its parameters (vo_pose_pair_end returns
 * what vo_pose_pair_ex with the same flags would have). */
int vo_pose_pair_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, int min_matches, double rigidity_thr,
                    double outlier_thr, int32_t* counts4, int32_t* rc2, double* T1_12, double* T2_12);
int vo_pose_pair_begin_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, int min_matches, double rigidity_thr,
                          double outlier_thr, int* ticket_out);

/* pose (stereo_odometer.py:82-105,177-223) ---------------------------------------------- */
/* cv2.estimateAffine3D(src, dst, force_rotation) Umeyama [:190,204]: T 3x4 row-major, scale */
int vo_umeyama(vo_ctx* ctx, const float* src /*m*3*/, const float* dst, int m, int force_rotation,
               double* T12, double* scale_out);
/* rigid_body_filter [:82-105] */
int vo_rigid_clique(vo_ctx* ctx, const float* prev, const float* cur, int m, double thr,
                    int64_t* mask_out /*m*/);
/* cv2.Rodrigues(R)[0] [:212]; host only */
int vo_rodrigues(const double* R9, double* r3);

/* RANSAC essential-matrix hypothesis scoring (BASELINE config 5) -------------------------------
 * NOT part of the reference (openVO has no RANSAC): defined by this build.  iters
 * hypotheses from 8-point minimal sets drawn by a counter-based hash RNG (seed), Sampson distance
 * (pixels, float32) against thr, inliers counted with wavefront ballot + popcount.  pts: n x 2
 * float32 pixel coordinates; K4 = fx, fy, cx, cy.  best2 = {winning hypothesis, its inlier count}
 * (ties -> lowest hypothesis index); mask_out (n) and counts_out (iters) may be NULL. */
int vo_ransac_essential(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K4, int iters,
                        float thr, uint32_t seed, double* E9_out, uint8_t* mask_out, int32_t* counts_out,
                        int32_t* best2_out);
/* Same contract with the five-point minimal solver (Nister 2004; the estimator cv2.findEssentialMat uses):
 * each hypothesis draws 6 correspondences, 5 give up to 10 essential matrices (float64, 10th-degree polynomial, real
 * roots isolated between derivative roots and bisected), the 6th picks the one with the smallest Sampson error; a
 * hypothesis without a real solution scores 0.  n >= 6. */
int vo_ransac_essential5(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K4, int iters,
                         float thr, uint32_t seed, double* E9_out, uint8_t* mask_out, int32_t* counts_out,
                         int32_t* best2_out);

/* Monocular front end of BASELINE config 5 (NOT part of the reference): vo_upload_mono puts one image into a slot
 * (vo_orb_detect_and_compute with mask_mode 0 then extracts its keypoints); vo_mono_pair chains, entirely on the
 * device and with ONE host synchronisation, Hamming kNN-2 between the two slots' descriptors -> ratio test ->
 * essential-matrix RANSAC (solver 8: as vo_ransac_essential, 5: as vo_ransac_essential5) on the survivors.  counts3 = {matches after the
 * ratio test, winning hypothesis, its inlier count}; E9_out = the winner; mask_out / q_idx / t_idx (each `cap`
 * entries, may be NULL): inlier flag, query and train keypoint index of the first counts3[0] entries. */
int vo_upload_mono(vo_ctx* ctx, int slot, const uint8_t* img, int w, int h, int channels);
/* look-ahead for a monocular stream: the left image of staged pair `index` into `slot` and its ORB extraction (mask_mode
 * 0) on a look-ahead engine's stream; a later vo_orb_detect_and_compute(slot, nfeatures, 0, ...) only waits for it */
int vo_prefetch_staged_mono(vo_ctx* ctx, int slot, int index, int nfeatures);
int vo_mono_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, const double* K4, int iters, float thr, uint32_t seed,
                 int solver, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap);
/* The same step in two halves, so that several pairs can be in flight (a monocular stream is latency-bound otherwise: each
 * pair's chain is short and narrow).  _begin enqueues the chain on one of VO_NUM_MONO_ASYNC alternates (own stream, scratch
 * and pinned result record), ordered behind whatever still produces the two slots, and returns a ticket; _end waits for that
 * ticket's completion event only and copies the record out.  want_matches != 0: mask / q / t and the second slot's keypoint
 * positions (xy_b_out: `cap` x 2 floats, may be NULL) travel with the record.  Results are those of vo_mono_pair, bit for bit.
 * A slot read by an open ticket may be refilled at any time: the refill is ordered behind the ticket's work on the device.
 * VO_E_STATE when every alternate is open. */
#define VO_NUM_MONO_ASYNC 5
/* 1 when the look-ahead work into `slot` (vo_prefetch_*) has finished or none is pending, 0 while it still runs; never blocks */
int vo_slot_ready(vo_ctx* ctx, int slot, int* ready_out);
int vo_mono_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, const double* K4, int iters, float thr, uint32_t seed,
                       int solver, int want_matches, int* ticket_out);
int vo_mono_pair_end(vo_ctx* ctx, int ticket, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx,
                     float* xy_b_out, int cap);
/* vo_mono_pair / vo_mono_pair_begin with match_flags (VO_MATCH_CROSSCHECK: kNN-2 -> ratio test -> cross-check -> RANSAC;
 * counts3[0] counts the matches that pass both tests) */
int vo_mono_pair_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                    uint32_t seed, int solver, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap);
int vo_mono_pair_begin_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                          uint32_t seed, int solver, int want_matches, int* ticket_out);

/* Monocular pose recovery on the device (NOT part of the reference) ------------------------------------------------------
 * vo_recover_pose: essential matrix + correspondences -> (R, unit t) with x2 ~ R x1 + t, the depths of the inliers and the ratio
 * of this pair's baseline to the previous pair's.  One launch of one block, host arrays in and out, one synchronisation.  Float64
 * throughout, no FMA contraction, three-term sums left to right; tests/mono_pose_ref.py restates it in numpy.
 *   E9 row-major; pts1 / pts2: n x 2 float32 pixels (1 <= n <= 65536); mask: n bytes (NULL: every point is an inlier); K4 = fx, fy,
 *   cx, cy; q_idx / t_idx (both or neither; NULL: the identity, na = nb = n): keypoint index of correspondence i in frame a / b;
 *   depth_a (may be NULL, na doubles): depth of frame a's keypoints in the PREVIOUS pair's units, a value that is not a positive
 *   finite number means none; min_parallax_sin2 >= 0.
 * Decomposition: E = U S Vt by one-sided Jacobi (signs flipped so that det U, det Vt > 0), R1 = U W Vt, R2 = U W^T Vt, t = U[:, 2].
 * Per correspondence and rotation, with x = (u - cx) / fx, h1 = (x1, 1), h2 = (x2, 1), a = R h1: nvec = h2 x t, d = a x h2,
 * dd = d.d, z1 = (nvec.d) / max(dd, 1e-300), z2 = ((z1 a + t).h2) / (h2.h2), sin2 = dd / ((a.a)(h2.h2)).
 * Vote over EVERY inlier: votes4 = {#(z1 > 0 and z2 > 0) for R1, #(z1 < 0 and z2 < 0) for R1, the same two for R2}: candidates
 * (R1, t), (R1, -t), (R2, t), (R2, -t).  The largest vote wins; on a tie the candidate whose R has the larger trace, then the
 * lower index.  Correspondence i is VALID when it is an inlier, z1 > 0, z2 > 0 and sin2 >= min_parallax_sin2 under the winner.
 * depth_b (may be NULL, nb doubles, written whole): z2 of the valid correspondence with the LOWEST i that names the keypoint,
 * 0 elsewhere.  z1_out / z2_out (may be NULL, n doubles): the winner's depths of the inliers, 0 for the others.
 * scale_rel: the lower median (rank (n_shared - 1) / 2, selected exactly) of depth_a[q_i] / z1_i over the n_shared valid
 * correspondences whose keypoint has a depth: |t_this| / |t_previous|; 0 when n_shared = 0.
 * out->flags  bit 0: no inlier, or a non-finite pose: R = I, t = 0, nothing but zeros written
 *             bit 1: an index outside [0, na) / [0, nb): nothing is read or written through it, the call returns VO_E_STATE
 *             bit 2: no scale: depth_a was NULL (vo_mono_pose_pair: the depths of slot a do not carry the serial asked for)
 * out->M = n, best_iter = -1, best_count = the number of inliers, serial = 0. */
typedef struct vo_mono_pose {
    int32_t M, best_iter, best_count;      /* matches after the ratio test (+ cross-check), winning hypothesis, its inliers */
    int32_t winner, n_depth, n_shared;     /* winning candidate 0 .. 3, valid correspondences, those with a depth in frame a */
    int32_t flags;
    uint32_t serial;                       /* of the step that wrote the record (and the depths of slot b) */
    int32_t votes4[4];
    double E[9], R[9], t[3], scale_rel;
} vo_mono_pose;                            /* 224 bytes */
int vo_recover_pose(vo_ctx* ctx, const double* E9, const float* pts1, const float* pts2, const uint8_t* mask, int n, const double* K4,
                    const int32_t* q_idx, const int32_t* t_idx, int na, int nb, const double* depth_a, double min_parallax_sin2,
                    vo_mono_pose* out, double* depth_b, double* z1_out, double* z2_out);
/* The monocular pair step with that tail instead of the per-match record: kNN-2 -> ratio (-> cross-check) -> hypotheses -> scores
 * as vo_mono_pair_ex, then ONE block: winner, its E and mask (as vo_mono_pair), vo_recover_pose on the surviving correspondences
 * with slot_a's keypoint depths, the record (a vo_mono_pose, nothing per match) written straight into pinned host memory.  No
 * further synchronisation and no copy command.  The depths land in slot_b (one double per keypoint) under the step's serial -- a
 * per-context counter that is never 0.  prev_serial: the serial of the step whose depths of slot_a may be used (0: none); when
 * slot_a's depths carry another serial, or the slot was refilled since, flag bit 2 is set and n_shared = 0, scale_rel = 0: never
 * a scale from another frame's or another reference's depths.  slot_a != slot_b.
 * _begin / _end: the same on a monocular alternate (tickets shared with vo_mono_pair_begin, VO_NUM_MONO_ASYNC in all; a ticket is
 * ended by the _end of the kind that began it).  A step begun ahead on (b, c) runs its kNN and RANSAC beside the step (a, b) that
 * writes b's depths and waits for it only before its own tail; a second writer of a slot's depths orders its tail behind the first. */
int vo_mono_pose_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                      uint32_t seed, int solver, uint32_t prev_serial, double min_parallax_sin2, vo_mono_pose* out);
int vo_mono_pose_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                            uint32_t seed, int solver, uint32_t prev_serial, double min_parallax_sin2, int* ticket_out,
                            uint32_t* serial_out);
int vo_mono_pose_pair_end(vo_ctx* ctx, int ticket, vo_mono_pose* out);
/* the keypoint depths a slot holds (out: one double per keypoint of the slot, vo_slot_num_keypoints; may be NULL) and their
 * serial (0: none, the depths then read 0); waits for the step that writes them */
int vo_download_mono_depth(vo_ctx* ctx, int slot, double* out, uint32_t* serial_out);

/* RANSAC solvePnP hypothesis scoring (north star; BASELINE config 2 names "ORB+SGBM+PnP") ----------
 * NOT part of the reference either (openVO fits 3-D/3-D, stereo_odometer.py:187-205): defined by this
 * build.  iters hypotheses; each draws 4 correspondences (same hash RNG), solves P3P on three of them in
 * float64 and lets the fourth pick among the <= 4 poses; P = K [R|t] in float32; a point is an inlier iff
 * it is in front of the camera and its reprojection error is below thr pixels (division-free float32
 * test), counted with wavefront ballot + popcount.  pts3d: n x 3 float32 (frame of the first view),
 * pts2d: n x 2 float32 pixels in the second view.  Rt12_out: row-major 3x4 world-to-camera pose of the
 * winner (ties -> lowest hypothesis index; all zeros if no hypothesis produced a pose). */
int vo_ransac_pnp(vo_ctx* ctx, const float* pts3d, const float* pts2d, int n, const double* K4, int iters,
                  float thr, uint32_t seed, double* Rt12_out, uint8_t* mask_out, int32_t* counts_out,
                  int32_t* best2_out);

/* Stereo PnP pair step (NOT part of the reference): what StereoOdometer(pose_method="pnp") computes per pair, for two
 * device-resident slots and with ONE host synchronisation: kNN-2 (+ ratio, + cross-check with VO_MATCH_CROSSCHECK) between the
 * two slots' descriptors -> 3-D lookup of the matched keypoints in slot_a (as vo_point_clouds) -> compaction of the usable
 * correspondences (status 0 and all three coordinates finite), pixels = slot_b's keypoint + the ROI origin (float32 add) ->
 * P3P RANSAC exactly as vo_ransac_pnp on those arrays (bit for bit) -> winner, mask [-> refine_iters (0 .. 20) Gauss-Newton
 * steps on the winner's inliers].
 *   counts4 = {M matches after the ratio test (and the cross-check), n usable correspondences, winning hypothesis, its inliers}
 *   flags   bit 0: a 3-D lookup in slot_a had no usable tap (the reference raises ZeroDivisionError); bit 1: a match index was
 *           outside the train set -- nothing is read through it and the call returns VO_E_STATE (a refused pair, never a wrong pose)
 *   Rt12    the winner as vo_ransac_pnp returns it (row-major 3x4); all zeros when n < 4 or no hypothesis produced a pose
 *   refine2 = {status, steps run}: 0 ok, 1 not requested or not attempted (fewer than 6 inliers), -1 the normal matrix was not
 *           positive definite or a value was not finite.  Rt12_refined (may be NULL) is valid only for status 0.
 *   mask_out / q_idx / t_idx (each `cap` >= slot_a's keypoint count entries, may be NULL): inlier flag, query and train keypoint
 *           index of the n usable correspondences (0 / -1 behind them).
 * The refinement, in float64: the inlier set is the winner's mask and stays fixed; residual (fx X'/Z' + cx - u, fy Y'/Z' + cy - v)
 * with X' = R X + t; a step sums J^T J and J^T r (d X'/d(w, v) = [-[X']x | I]) in a fixed order, solves the 6x6 system by
 * Cholesky and updates R <- Exp(w) R, t <- Exp(w) t + v; exactly refine_iters steps, no early exit: a function of the inputs alone. */
int vo_pnp_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                uint32_t seed, int refine_iters, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
                int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap);
/* The same step in two halves, as vo_pose_pair_begin / _end.  The tickets ARE pose tickets: they come from the same
 * VO_NUM_POSE_ASYNC alternates and run on the same three streams, so that number bounds the open pose and PnP steps together;
 * a ticket is ended by the _end of the kind that began it (VO_E_STATE otherwise).  want_matches != 0: mask / q / t travel with
 * the record.  _end checks both slots' disparity health (VO_E_SWEEP) like vo_pose_pair_end and delivers what vo_pnp_pair would
 * have, bit for bit.  A slot read by an open ticket may be refilled at any time. */
int vo_pnp_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                      uint32_t seed, int refine_iters, int want_matches, int* ticket_out);
int vo_pnp_pair_end(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                    uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap);
/* The PnP step with local-optimisation rounds (LO-RANSAC): the refit re-selects its inliers.  tests/pnp_lo_ref.py restates it.
 * With the winner Rt_0 (float64), its mask S_0, the n usable correspondences X / uv (float32), K4, thr (float32), steps =
 * refine_iters (1 .. 20) and R = lo_rounds (1 .. 8), for r = 1 .. R:
 *   1. (Rt_r, status) = the refinement above from Rt_{r-1} on the set S_{r-1}, `steps` steps: the same arithmetic.  Status 1: fewer
 *      than 6 points in S_{r-1}; -1: a pivot was not positive or a value was not finite.
 *   2. status != 0: the round is discarded entirely and the loop ends.
 *   3. S_r[i], for every i < n, = the scoring kernels' own test under Rt_r: P = K [R | t] rounded to float32 the way a
 *      hypothesis's P is formed -- (float)(fx Rt[c] + cx Rt[8 + c]), (float)(fy Rt[4 + c] + cy Rt[8 + c]), (float)Rt[8 + c] for
 *      c = 0 .. 3 -- then the division-free float32 test of vo_ransac_pnp against thr * thr.
 * The result is (Rt_c, S_c) of the last completed round c = 0 .. R; status 0 when c >= 1, otherwise round 1's status, which is
 * the plain refinement's for the same inputs.  No early exit, no acceptance test: a function of the inputs alone.  With R = 1 the
 * pose is vo_pnp_pair's Rt12_refined, bit for bit.
 *   lo_rounds 0 .. 8; a value >= 1 needs refine_iters >= 1 (VO_E_ARG otherwise).  lo_rounds == 0: every output equals the plain
 *           entry's, bit for bit, and lo2 = {0, best_count}.
 *   lo2     = {rounds completed c, |S_c|}
 *   counts4, Rt12, q_idx, t_idx: unchanged -- the RANSAC's own result stays inspectable.  mask_out: S_c.  Rt12_refined: the LO pose
 *           Rt_c, valid for status 0.  refine2 = {status, Gauss-Newton steps applied in the completed rounds (c * refine_iters)}.
 * The rounds are part of a ticket's parameters; either _end ends a PnP ticket of either kind, the plain one returns no lo2. */
int vo_pnp_pair_lo(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                   uint32_t seed, int refine_iters, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
                   int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds, int32_t* lo2);
int vo_pnp_pair_begin_lo(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4, int iters, float thr,
                         uint32_t seed, int refine_iters, int want_matches, int lo_rounds, int* ticket_out);
int vo_pnp_pair_end_lo(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                       uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int32_t* lo2);

/* Sparse stereo depth (NOT part of the reference, which reads a dense disparity at its keypoints, stereo_odometer.py:50-79,117):
 * per-keypoint 3-D from ORB on BOTH rectified images of a slot, without any SGBM run.  Defined by this build; tests/sparse_stereo_ref.py
 * restates steps b - e in numpy.  Needs a pair in the slot (vo_upload_pair / vo_load_staged_pair) and vo_set_Q; one host synchronisation
 * (a slot filled by a vo_prefetch_*_sparse entry: see there).
 *   a. KL = ORB(left crop), KR = ORB(right crop): the crop rectangle of vo_orb_detect_and_compute (from the LEFT ROI) on both images,
 *      no mask, canonical order, nfeatures each.
 *   b. association of left keypoint i: right keypoint j is a candidate when |oct_i - oct_j| <= 1, fabsf(y_i - y_j) <= row_tol * sc[oct_i]
 *      (sc[o] = (float)pow((double)1.2f, o)) and d0 = x_i - x_j (float32) lies in [min_disp, max_disp]; the winner is the
 *      lexicographically smallest (Hamming distance, j), accepted when its distance <= max_hamming.
 *   c. refinement in crop pixels: x0 = rint(x_i), y0 = rint(y_i), xr = rint(x_j) (half to even); rejected when the 11 x 11 window at
 *      (x0, y0) or the 11 x 21 strip around (xr, y0) leaves the crop; SAD(s) = sum |L[y0+dy, x0+dx] - R[y0+dy, xr+s+dx]| for s = -5 .. 5
 *      in integers; s* = the first minimum, rejected at s* = +-5; den = SAD(s*-1) + SAD(s*+1) - 2 SAD(s*), rejected when den <= 0;
 *      delta = (float)(SAD(s*-1) - SAD(s*+1)) / (float)(2 den); d = (float)(x0 - xr - s*) - delta; kept iff d > 0 and
 *      min_disp <= d <= max_disp.
 *   d. 3-D: cv2.reprojectImageTo3D's arithmetic (as vo_download_xyz) on v = {(double)(x_i + (float)roi_x0), (double)(y_i + (float)roi_y0),
 *      (double)d, 1}, the additions in float32.
 *   e. the surviving LEFT keypoints, in their order, become the slot's keypoints (all six arrays and the descriptors) together with
 *      their 3-D point and disparity; the slot's keypoints then CARRY DEPTH until the next ORB extraction into the slot or its refill.
 * 0 <= min_disp < max_disp, row_tol >= 0 (finite float32), max_hamming 0 .. 256, VO_E_ARG otherwise; more than 65535 right keypoints:
 * VO_E_CAP.  counts3 = {left keypoints, accepted associations, kept}. */
int vo_sparse_stereo(vo_ctx* ctx, int slot, int nfeatures, float min_disp, float max_disp, float row_tol, int max_hamming,
                     int32_t* counts3);
/* the 3-D points (n x 3) and disparities (n) of a slot's keypoints, in keypoint order; either output may be NULL.  VO_E_STATE when the
 * slot's keypoints carry no depth. */
int vo_download_keypoint_depth(vo_ctx* ctx, int slot, float* xyz /*cap*3*/, float* disp /*cap*/, int cap, int* n_out);
/* Association tests of step b (two EXTENSIONS of it, both off by default; tests/sparse_loop_ref.py restates them).  Candidates,
 * distances and the key (distance << 16 | j) are those of step b.
 *   VO_SPARSE_RATIO: (d1, j1) and (d2, j2) are the two lexicographically smallest (distance, j) among ALL candidates of left keypoint
 *     i, the second whatever its distance.  i is accepted iff d1 <= max_hamming and (there is no second candidate or
 *     (float)d1 < ratio * (float)d2, in float32): d1 == d2 fails for every legal ratio, a single candidate passes.  A keypoint that
 *     fails has match -1 and is not refined.
 *   VO_SPARSE_MUTUAL: a(j) = the lexicographically smallest (distance, i) over the left keypoints i that have j as a candidate at a
 *     distance <= max_hamming (whether or not j is their winner).  A left keypoint i accepted with match j survives iff a(j) names
 *     i; one that does not has match -1 and disparity NaN.  The key is (distance << 16 | i): more than 65535 left keypoints with
 *     this bit set is VO_E_CAP.
 * counts3[1] counts the associations that pass the threshold and every enabled test; counts3[2] what survives the refinement too.
 * The tests are context state, read when a sparse chain is ENQUEUED (vo_sparse_stereo and the vo_prefetch_*_sparse entries) and
 * part of the request from then on: a chain begun ahead under another state is recomputed by vo_sparse_stereo exactly as one begun
 * with another row_tol.  ratio is read only with VO_SPARSE_RATIO and must then satisfy 0 < ratio <= 1; any other bit of flags, or
 * such a ratio, is VO_E_ARG.  flags = 0 is the association of step b alone. */
#define VO_SPARSE_MUTUAL 1
#define VO_SPARSE_RATIO 2
int vo_set_sparse_assoc(vo_ctx* ctx, int flags, float ratio);
/* the descriptor (32 bytes) of the RIGHT keypoint each of a slot's keypoints was associated with, in keypoint order (its position is
 * (x - disparity, about y)); valid exactly while the keypoints carry depth: VO_E_STATE otherwise.  rdesc may be NULL (the count only). */
int vo_download_keypoint_rdesc(vo_ctx* ctx, int slot, uint8_t* rdesc /*cap*32*/, int cap, int* n_out);
/* steps b and c on host arrays, no ORB involved (the seam the kernel tests use): two w x h images (the crop is the whole image),
 * nl / nr keypoints (x, y pairs, octaves 0 .. 7, 32-byte descriptors).  match_out[i] = the accepted right keypoint or -1;
 * disp_out[i] = d, NaN where keypoint i was not accepted or was rejected by the refinement. */
int vo_sparse_match_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l, const int32_t* oct_l,
                         const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r, const uint8_t* desc_r, int nr,
                         float min_disp, float max_disp, float row_tol, int max_hamming, int32_t* match_out /*nl*/, float* disp_out /*nl*/);
/* steps b - e on host arrays in ONE launch (k_sparse_pair: association and refinement, then the compaction in the workgroup that
 * arrives last; the seam that kernel's tests use): vo_sparse_match_host's inputs plus Q and the ROI origin of step d.  match_out /
 * disp_out as there; the survivors, in their order, come back as kp_xy / kp_octave / desc / kp_disp / kp_xyz (nl entries of room each),
 * compacted into a destination that is not the scratch set they are read from.  counts3 as vo_sparse_stereo. */
int vo_sparse_pair_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l, const int32_t* oct_l,
                        const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r, const uint8_t* desc_r, int nr,
                        float min_disp, float max_disp, float row_tol, int max_hamming, const double* Q16, int roi_x0, int roi_y0,
                        int32_t* match_out /*nl*/, float* disp_out /*nl*/, float* kp_xy /*nl*2*/, int32_t* kp_octave /*nl*/,
                        uint8_t* desc /*nl*32*/, float* kp_disp /*nl*/, float* kp_xyz /*nl*3*/, int32_t* counts3);
/* the same with the association tests as arguments (assoc_flags / assoc_ratio as vo_set_sparse_assoc; the context's state is neither
 * read nor changed) and one more output: kp_rdesc, the descriptor of right keypoint match[i] of every survivor (may be NULL).
 * vo_sparse_pair_host is this entry with assoc_flags 0. */
int vo_sparse_pair_host_ex(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l, const int32_t* oct_l,
                           const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r, const uint8_t* desc_r, int nr,
                           float min_disp, float max_disp, float row_tol, int max_hamming, int assoc_flags, float assoc_ratio,
                           const double* Q16, int roi_x0, int roi_y0, int32_t* match_out /*nl*/, float* disp_out /*nl*/,
                           float* kp_xy /*nl*2*/, int32_t* kp_octave /*nl*/, uint8_t* desc /*nl*32*/, float* kp_disp /*nl*/,
                           float* kp_xyz /*nl*3*/, uint8_t* kp_rdesc /*nl*32*/, int32_t* counts3);
/* Sparse stereo begun ahead (NOT part of the reference either).  The three entries are vo_prefetch_pair / vo_prefetch_host_staged /
 * vo_prefetch_staged_pair with the sparse stereo chain in place of the SGBM: on the next look-ahead engine's stream the pair is
 * ingested into the slot, both extractions run as one batch, and one launch associates, refines and compacts; the slot's `ready` is
 * recorded behind it and the slot counts towards vo_lookahead_depth.  The request (the five trailing arguments, as vo_sparse_stereo)
 * is checked before anything is enqueued; vo_set_Q is needed, vo_set_sgbm is not, and an engine that only ever sees sparse pairs
 * never allocates an SGBM workspace.  The slot then holds the pair, no disparity and -- until collected -- no keypoints:
 *   vo_sparse_stereo(slot, the same request) launches nothing: it waits for the slot (a host wait on its event, as
 *     vo_orb_detect_and_compute does for keypoints extracted ahead), reads the slot's own record, applies vo_sparse_stereo's capacity
 *     checks and returns counts3; the results are bit for bit those of the synchronous call.  With another request it waits and
 *     recomputes synchronously from the slot's pair.  On a slot begun ahead that has already been collected with the same request it
 *     returns the counts again without recomputing; nothing else is ever reused: a result computed synchronously is recomputed by
 *     the next call, as before, and vo_set_Q / vo_set_roi void both a pending chain and a collected one (the next call computes
 *     with the Q and ROI in force).
 *   An ORB extraction into the slot or a refill before that voids the chain's result, like the depth mark itself.
 *   The pair steps (vo_pose_pair_begin, vo_pnp_pair_begin, ...) need COLLECTED slots: VO_E_STATE otherwise. */
int vo_prefetch_pair_sparse(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h, int channels, int preprocessed,
                            int nfeatures, float min_disp, float max_disp, float row_tol, int max_hamming);
int vo_prefetch_host_staged_sparse(vo_ctx* ctx, int slot, int buf, int w, int h, int channels, int preprocessed, int nfeatures,
                                   float min_disp, float max_disp, float row_tol, int max_hamming);
int vo_prefetch_staged_pair_sparse(vo_ctx* ctx, int slot, int index, int preprocessed, int nfeatures, float min_disp, float max_disp,
                                   float row_tol, int max_hamming);
/* The pair steps read their depth source from the slots: when BOTH slots' keypoints carry depth, vo_point_clouds(_ex),
 * vo_pose_pair(_ex / _begin / _begin_ex / _end) and vo_pnp_pair(_begin / _end) take the 3-D point of keypoint k from the slot's
 * per-keypoint array instead of the bilinear lookup in the reprojected disparity (status 0; the slots need no disparity and its
 * health is not consulted); when neither does, nothing changes; when exactly one does, VO_E_STATE. */

/* Landmark map (NOT part of the reference, whose every pose is the pose of one pair of frames, stereo_odometer.py:115-160): up to
 * `capacity` landmarks resident on the device, so that a frame can be tracked against a local map instead of against the previous
 * frame (StereoOdometer(track="map")).  Defined by this build; tests/map_ref.py restates both kernels in numpy.  A landmark is
 * xyz (3 x float32, WORLD coordinates = the camera frame of the first tracked frame), desc (32 B), rdesc (32 B: the right-image
 * partner's descriptor of its last observation, so that VO_MATCH_LOOP works on a view), octave, obs (observations so far) and last
 * (serial of the frame that last observed it).  A map is an int handle inside the context, at most VO_NUM_MAPS per context; every
 * byte of it is allocated by vo_map_create (two sets of the arrays: an update compacts from one into the other, never in place),
 * nothing on the per-frame path.  16 <= capacity <= kp_cap (= 2 max_kp + 1024), so that a view always fits a frame slot.
 * With T(Rt, p)[i] = (float)(((R[i][0] * (double)p.x + R[i][1] * (double)p.y) + R[i][2] * (double)p.z) + t[i]), R | t the row-major
 * 3x4 Rt:
 *
 * vo_map_view (one launch of one workgroup, ONE host synchronisation): the map as seen under the world-to-camera pose Rt12_cw
 *   becomes the keypoints of view_slot.  For landmark l in map order: Xc = T(Rt12_cw, xyz[l]);
 *   u = (float)(fx * ((double)Xc[0] / (double)Xc[2]) + cx) - (float)roi_x0, v likewise with fy, cy, roi_y0 (float32 subtractions);
 *   K4 = fx, fy, cx, cy in full-image pixels as vo_pnp_pair takes it; the ROI origin and the crop (crop_w x crop_h) are those
 *   vo_orb_detect_and_compute uses for ref_slot's image -- ref_slot is the frame that will be matched against the view and must
 *   hold an image (VO_E_STATE otherwise).  l is VISIBLE iff Xc is finite in all three, Xc[2] >= z_min, 0 <= u <= (float)(crop_w - 1)
 *   and 0 <= v <= (float)(crop_h - 1).  The visible landmarks, in map order, are view_slot's keypoints: position (u, v), 3-D point
 *   Xc (CAMERA coordinates: what the PnP step sees stays small however far the camera has travelled, and its result is the motion
 *   from Rt12_cw to the new frame), desc, right descriptor, octave; size = angle = response = 0, disparity NaN.  The slot then
 *   stands as vo_sparse_stereo leaves one (keypoints that carry depth; nothing pending or begun ahead; no request equals its
 *   own), ordered behind whatever still reads or writes it.  Which landmark each keypoint came from is kept with the map (the LAST
 *   VIEW) for vo_map_update.  counts2 = {map size, visible}.  z_min finite >= 0, every entry of Rt12_cw / K4 finite, fx, fy > 0,
 *   view_slot != ref_slot: VO_E_ARG otherwise.
 *
 * vo_map_update (one launch of one workgroup, ONE host synchronisation): folds the tracked frame in slot_new (whose keypoints must
 *   carry depth: VO_E_STATE otherwise) into the map.  q_idx / t_idx / mask (n entries each, host arrays; NULL only with n = 0) are
 *   what vo_pnp_pair(view_slot, slot_new, ...) delivered: q indexes the last view, t slot_new's keypoints.  Rt12_wc = the
 *   camera-to-world pose of slot_new.  Checked on the host before anything is enqueued (VO_E_ARG): 0 <= n <= kp_cap, every
 *   0 <= q < the last view's count (0 after an update, a reset or no view yet), every 0 <= t < slot_new's keypoints, no q twice among
 *   the entries with mask != 0, max_age >= 0, 1 <= max_obs <= 65535, serial >= 0 and >= every serial used since the last reset,
 *   every entry of Rt12_wc finite.
 *   1. observations: for every c with mask[c] != 0, l = the landmark of view keypoint q[c], t = t_idx[c], Xo = T(Rt12_wc, the 3-D
 *      point of keypoint t).  Xo not finite: the landmark is left alone (counted as skipped).  Otherwise m = min(obs[l], max_obs),
 *      xyz[l][i] = (float)((double)xyz[l][i] + ((double)Xo[i] - (double)xyz[l][i]) / (double)(m + 1)) -- a running mean whose
 *      weight stops shrinking at 1 / (max_obs + 1) --, obs[l] += 1, last[l] = serial, desc / rdesc / octave from keypoint t, and t
 *      is CLAIMED (several landmarks may claim one t: each takes its own observation).
 *   2. survivors: the landmarks with serial - last[l] <= max_age, in their order; the others are counted as culled.
 *   3. insertions: the unclaimed keypoints t of slot_new with a finite Xo, in keypoint order, enter behind the survivors with
 *      xyz = Xo, obs = 1, last = serial until `capacity` is reached; the rest are counted as dropped (an unclaimed keypoint
 *      without a finite point is neither).
 *   4. the other set of arrays becomes the map; the last view is void.
 *   counts6 = {observed, skipped, culled, inserted, dropped, size}.  n = 0 is insert-and-age only: how a first frame fills the map.
 *
 * With vo_enable_timing on, the view's launch is bracketed under VO_T_MATCH and the update's under VO_T_POSE.
 * A refused call leaves the map as it was.  vo_map_reset: size 0, no view, serials start over.  vo_map_download: the landmarks in
 * map order (any output may be NULL; VO_E_CAP when cap is below the size).  A fifth map: VO_E_CAP.
 *
 * vo_track_map (ONE host synchronisation; tests/map_fused_ref.py restates it): vo_map_view + vo_pnp_pair(view_slot, slot_new) +
 *   the odometer's decisions and motion gates + vo_map_update as one chain of launches on the context's stream; nothing but the
 *   record (and q / t / mask when asked for) comes back.  With n = the map's size as the host knows it and vis = the visible count, which only the device knows:
 *   a. padded view: rows [0, vis) of view_slot are exactly vo_map_view's keypoints under Rt12_cw_pred (ref_slot = slot_new), and
 *      view_src is written as there.  Rows [vis, n) are PADDING so that the later launches can be shaped for n: clones of row 0
 *      in position, octave, descriptor and right descriptor, with a NaN 3-D point (size = angle = response = 0, disparity NaN as
 *      every view row).  With vis = 0 the padding's position, octave and descriptors are zero.
 *   b. kNN-2 with n query rows (match_flags as vo_pnp_pair).  A clone ties with row 0 in every column minimum of the cross-check
 *      and loses to it (the lower query index wins), and under VO_MATCH_WINDOW carries row 0's pixel: rows [0, vis) get the
 *      results of the compacted view.  The ratio test and everything behind it see the first vis rows only, so M, n_usable, the
 *      RANSAC and the refinement are those of vo_pnp_pair on vo_map_view's slot, bit for bit.
 *   c. decision, the first that applies (Rt = Rt12_refined when the refinement's status is 0, else the winner; mm = min_matches):
 *        1  vis < max(mm, 2) or vis > 3800         the view is refused (no skip cause: the caller falls back)
 *        2  M < mm                                   "matches"
 *        8  flag bit 1 of the PnP step             a match index outside the train set: the call returns VO_E_STATE
 *        3  n_usable < max(mm, 4)                    "matches"
 *        4  best_count < mm                          "outlier"
 *        5  an entry of Rt is NaN                    "nan"
 *        6  |t| > max_dist (and not 7)               "bigdist"
 *        7  angle > max_rot                          "bigrot"
 *        0  otherwise: accepted
 *      |t| = sqrt((t0 t0 + t1 t1) + t2 t2); angle = atan2(s, c), s = sqrt((a a + b b) + c' c') / 2 over (a, b, c') = (R32 - R23,
 *      R13 - R31, R21 - R12), c = (((R11 + R22) + R33) - 1) / 2, all float64.  max_dist / max_rot are the caller's gates already
 *      multiplied by the frames the step spans.
 *   d. on 0: c_T_w = Rt . Rt12_cw_pred as 4x4 products, entry (i, j) = ((Rt[i][0] P[0][j] + Rt[i][1] P[1][j]) + Rt[i][2] P[2][j]) +
 *      Rt[i][3] P[3][j] with P's last row (0, 0, 0, 1), no fused multiply-add; w_T_c = [R^T | -(R^T t)] of it, row i of the last
 *      column = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2).  Then vo_map_update's steps 1 - 4 with Rt12_wc = w_T_c and the n_usable
 *      correspondences of b (q, t, mask), all read from device memory; the kernel makes the range checks itself (q < vis, t <
 *      slot_new's keypoints, as unsigned compares): one violation and nothing is applied, bit 0 of update_flags is set and the call
 *      returns VO_E_STATE.  On any other decision the six counts are -1 and the map is not touched.
 *   Afterwards view_slot stands exactly as vo_map_view leaves it (vis keypoints); on 0 the other set of arrays is the map and the
 *   last view is void, otherwise the last view is this one.  mask_out / q_idx / t_idx as vo_pnp_pair (cap >= n, any may be NULL).
 *   Checked before anything is enqueued: vo_map_view's arguments (ref_slot = slot_new), vo_pnp_pair's, vo_map_update's serial /
 *   max_age / max_obs / depth-carrying slot_new, min_matches >= 0, max_dist and max_rot not NaN; a map of more than 3800 landmarks
 *   is VO_E_CAP (the fused PnP step's bound applies to n).  A refused call leaves the map as it was.
 *   With vo_enable_timing on: the padded view is one bracket under VO_T_MATCH, the decision and the update one each under VO_T_POSE. */
#define VO_NUM_MAPS 4
#define VO_MAP_TRACK_MAX 3800
typedef struct vo_track_map_rec {
    int32_t decision, map_n, vis, update_flags;
    int32_t M, n, best_iter, best_count;       /* counts4 of vo_pnp_pair */
    int32_t flags, rstatus, rsteps, pad;       /* its flags and refine2 */
    int32_t counts6[6], pad2[2];               /* vo_map_update's counts; -1 each unless decision == 0 */
    double Rt[12], Rtr[12];                    /* its Rt12 and Rt12_refined */
    double c_T_w[12], w_T_c[12];               /* the new world-to-camera pose and its inverse (decision == 0; zeros otherwise) */
} vo_track_map_rec;
int vo_track_map(vo_ctx* ctx, int map, int slot_new, int view_slot, const double* Rt12_cw_pred, const double* K4, float z_min,
                 double ratio, int match_flags, int iters, float thr, uint32_t seed, int refine_iters,
                 int min_matches, double max_dist, double max_rot, int serial, int max_age, int max_obs,
                 vo_track_map_rec* rec, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap);
/* vo_track_map with the PnP step of vo_pnp_pair_lo (lo_rounds as there; 0: this IS vo_track_map).  The decisions, the gates and the
 * composition of c / d see the LO pose when its status is 0 (decision 4 still reads the winner's best_count); step 1 of the update
 * reads S_c; mask_out is S_c.  The record keeps its size and offsets: rec->pad = rounds completed, rec->pad2[0] = |S_c| (both 0
 * with lo_rounds == 0). */
int vo_track_map_lo(vo_ctx* ctx, int map, int slot_new, int view_slot, const double* Rt12_cw_pred, const double* K4, float z_min,
                    double ratio, int match_flags, int iters, float thr, uint32_t seed, int refine_iters,
                    int min_matches, double max_dist, double max_rot, int serial, int max_age, int max_obs,
                    vo_track_map_rec* rec, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds);
int vo_map_create(vo_ctx* ctx, int capacity, int* map_out);
int vo_map_destroy(vo_ctx* ctx, int map);
int vo_map_reset(vo_ctx* ctx, int map);
int vo_map_view(vo_ctx* ctx, int map, const double* Rt12_cw, const double* K4, float z_min, int ref_slot, int view_slot,
                int32_t* counts2);
int vo_map_update(vo_ctx* ctx, int map, int slot_new, const double* Rt12_wc, int serial, int max_age, int max_obs,
                  const int32_t* q_idx, const int32_t* t_idx, const uint8_t* mask, int n, int32_t* counts6);
int vo_map_download(vo_ctx* ctx, int map, float* xyz /*cap*3*/, uint8_t* desc /*cap*32*/, int32_t* octave, int32_t* obs, int32_t* last,
                    int cap, int* n_out);

/* Lucas-Kanade tracking (NOT part of the reference, whose every temporal association is a descriptor match,
 * stereo_odometer.py:162-175): pyramidal KLT with a forward-backward check, the front end of StereoOdometer(match="klt").  Defined by
 * this build, operation by operation, so that the kernels are held bit for bit to tests/klt_ref.py; parity with OpenCV's
 * calcOpticalFlowPyrLK (whose fixed-point variant differs in its tap weights and border rule) is not claimed.  Integer stages are
 * exact; the scalar step is float64 in the order written below, every product and sum rounded on its own (no fused multiply-add).
 *   Parameters: win odd, 5 .. 31; levels 1 .. 6; iters 1 .. 100; eps, min_eig, fb finite and >= 0 (fb = 0: no forward-backward
 *   check).  The defaults of the Python layer are 21, 4, 30, 0.01, 1e-4, 1.0.
 *   Pyramid: level 0 is the u8 image; level l + 1 has size ((w + 1) / 2, (h + 1) / 2) and pixel (x, y) =
 *   (sum_{i, j = -2 .. 2} k[i] k[j] I[r(2 y + j)][r(2 x + i)] + 128) >> 8 with k = 1 4 6 4 1 and r the reflection that does not repeat
 *   the edge: |i| below 0, 2 (n - 1) - i past the end (clamped to the image afterwards, which only acts on an image narrower than 3).
 *   Reads: a read of a level at (x, y) is the pixel at (clamp(x, 0, w - 1), clamp(y, 0, h - 1)): none is out of bounds, none is
 *   refused.  Gradient at the integer pixel (x, y), on such reads, as integers: Dx = 3 (I[y-1][x+1] - I[y-1][x-1]) +
 *   10 (I[y][x+1] - I[y][x-1]) + 3 (I[y+1][x+1] - I[y+1][x-1]), Dy the transpose of it.
 *   Window at the real position c (win x win): t = c - (win - 1) / 2, i = floor(t) (as an integer, saturated at +-2^30), f = t -
 *   floor(t), per axis, in float64; w00 = rint(((1 - fx) (1 - fy)) 16384), w01 = rint((fx (1 - fy)) 16384), w10 = rint(((1 - fx) fy) 16384)
 *   (half to even), w11 = 16384 - w00 - w01 - w10.  Window pixel (u, v), with x = ix + u, y = iy + v: image sample =
 *   (w00 I[y][x] + w01 I[y][x+1] + w10 I[y+1][x] + w11 I[y+1][x+1] + 256) >> 9 (5 fractional bits); gradient sample = the same four
 *   taps of Dx (Dy), (... + 8192) >> 14, arithmetic shifts.
 *   Per point: a non-finite input has status 4, is returned as it came and reads nothing.  Otherwise p0 = (double)xy + origin (the
 *   origin is 0 for vo_klt_track_host and the ROI origin for vo_klt_track), q = p0 / 2^(levels - 1), and for L = levels - 1 .. 0, on
 *   level L of both pyramids:
 *     template I, Dx, Dy = the samples of image A at p0 / 2^L; A11 = sum Dx Dx, A12 = sum Dx Dy, A22 = sum Dy Dy in integers, then
 *     as doubles (exact); D = A11 A22 - A12 A12; with s = 2^-20:
 *     minEig = ((A22 + A11) s - sqrt(((A11 - A22) s) ((A11 - A22) s) + (4 (A12 s)) (A12 s))) / (2 win win).
 *     minEig < min_eig or D <= 0: the level is skipped (at L = 0: status bit 1).  Otherwise at most iters iterations k = 1, 2, ...:
 *       unless -win <= qx <= (wL - 1) + win and -win <= qy <= (hL - 1) + win the point is LOST: status bit 2, q = q 2^L, nothing
 *       further is computed for it;
 *       the iteration counts; J = the image samples of B at q; b1 = sum (J - I) Dx, b2 = sum (J - I) Dy in integers, then doubles;
 *       dx = (A12 b2 - A22 b1) / D, dy = (A12 b1 - A11 b2) / D; q = q + (dx, dy);
 *       dx dx + dy dy <= eps eps: the level ends;
 *       otherwise, for k >= 2, |dx + dx_prev| < 0.01 and |dy + dy_prev| < 0.01 (an oscillation): q = q - 0.5 (dx, dy), the level ends.
 *     Behind every level but the last, q = 2 q.
 *   A point that was not lost on the way gets status bit 2 unless 0 <= qx <= w - 1 and 0 <= qy <= h - 1.
 *   Outputs, per point: xy_out = (float)(q - origin); status_out = 0 tracked | 1 eigenvalue at level 0 | 2 left the image |
 *   4 non-finite input | 8 forward-backward; iters_out = the iterations that counted, over all levels and both directions.
 *   Forward-backward (fb > 0): every point with status 0 is tracked from B to A in the same way, starting at xy_out as float32;
 *   with (x', y') its float32 result and (x, y) the float32 input, d2 = (x' - x)(x' - x) + (y' - y)(y' - y) in float64; the point keeps
 *   status 0 iff the backward track has status 0 and d2 <= fb fb, and gets bit 8 otherwise; xy_out stays the forward result.
 * Both entries are synchronous on the context's stream; with vo_enable_timing on, the pyramid launches are bracketed under VO_T_ORB
 * and the tracking launches under VO_T_MATCH.  The two pyramids live in the Lucas-Kanade workspace of the context's main match scratch
 * (allocated at the first call from max_w, max_h and the keypoint capacity, freed by vo_destroy; nothing is allocated per call; a
 * pose alternate that runs vo_klt_pnp_pair_begin owns another) and are rebuilt by every call.
 * vo_klt_track_host: two w x h host images and n points in full-image coordinates (0 <= n <= keypoint capacity = 2 max_kp + 1024;
 *   n = 0 is valid and launches nothing).  A bad parameter, a NULL pointer or n < 0: VO_E_ARG; w / h above max_w / max_h or n above
 *   the capacity: VO_E_CAP; nothing is launched and no output is written by a refused call.
 * vo_klt_track: slot_a's keypoints (ROI-cropped coordinates, as every keypoint of a slot) from slot_a's rectified left image into
 *   slot_b's; the ROI origin is added in float64 on the way in and subtracted before the float32 rounding on the way out, the images
 *   are the whole rectified images (a track may leave the crop and stay inside the image).  The call orders itself behind whatever
 *   still writes either slot, as vo_point_clouds_ex does, and registers nothing that outlives it.  *n_out = slot_a's keypoint count
 *   (VO_E_CAP when cap is below it; iters_out may be NULL).  VO_E_STATE: no pair in a slot, no keypoints in slot_a, or two slots of
 *   different shapes. */
int vo_klt_track_host(vo_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, const float* xy /*n*2*/, int n, int win,
                      int levels, int iters, double eps, double min_eig, double fb, float* xy_out /*n*2*/, uint8_t* status_out /*n*/,
                      int32_t* iters_out /*n*/);
int vo_klt_track(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int iters, double eps, double min_eig, double fb,
                 float* xy_out /*cap*2*/, uint8_t* status_out /*cap*/, int32_t* iters_out /*cap*/, int cap, int* n_out);

/* Lucas-Kanade PnP pair step (an extension, NOT part of the reference): vo_klt_track -> the filter "status 0" -> the 3-D points
 * of the kept keypoints in slot_a -> vo_ransac_pnp, value for value, as ONE chain of launches on the context's stream with ONE
 * host synchronisation and no copy command: the pyramid launches, the forward (fb > 0: and the backward) tracking launch,
 * k_klt_pnp_prep, k_pnp_hyp, k_pnp_score, k_pnp_finish.  Nothing per keypoint is downloaded unless an array is asked for.
 *   win .. fb: the tracker's parameters (klt_iters = its iteration limit), as vo_klt_track takes them.  K4, iters, thr, seed,
 *   refine_iters: as vo_pnp_pair.  lo_rounds: as vo_pnp_pair_lo (0: the plain refit).
 *   The 3-D point of keypoint i: slot_a's kp_xyz[i] where its keypoints carry depth (vo_sparse_stereo), else the bilinear lookup
 *   of vo_points3d_at at the keypoint in slot_a's disparity.  A track is dropped -- never an error -- where that lookup has no
 *   usable tap (flag bit 0 says that it happened), status 1, or a coordinate that is not finite.
 *   counts4 = {M, n, best_iter, best_count}: M = tracks with status 0, n = correspondences that reached the RANSAC (n < 4: no pose,
 *   best (0, 0), Rt all zero).  *flags: bit 0 as above, bit 1 never.  Rt12, Rt12_refined, refine2, lo2 (may be NULL): as
 *   vo_pnp_pair_lo.  mask_out, q_idx, xy_out (each may be NULL; cap entries, cap >= slot_a's keypoint count or VO_E_CAP): per
 *   compacted correspondence, in keypoint order, the winner's inlier byte (the set S_c behind completed rounds), the keypoint
 *   index, and the tracked position in slot_b's ROI-cropped pixels as vo_klt_track returns it (the RANSAC was given that position
 *   plus the ROI origin, a float32 add); q_idx reads -1 and mask_out 0 from n to the keypoint count, xy_out is written up to n.
 *   VO_E_ARG: a bad slot or pointer, a tracker parameter vo_klt_track refuses, iters, thr, refine_iters or a focal length
 *   vo_pnp_pair refuses, lo_rounds outside 0 .. 8 or above 0 without refine_iters.  VO_E_STATE: no pair in a slot, no keypoints in
 *   slot_a (a slot whose extraction found none is fine: the cleared record, nothing launched), two slots of different shapes,
 *   slot_a with neither disparity nor depth-carrying keypoints, no vo_set_Q.  slot_b needs neither keypoints nor disparity.
 *   VO_E_SWEEP: slot_a's disparity is undefined.  A refused call launches nothing and writes no output.
 * vo_klt_pnp_pair_begin / _end: the same step in two halves on a POSE alternate (the tickets, streams and scratch of
 * vo_pose_pair_begin and vo_pnp_pair_begin: VO_NUM_POSE_ASYNC bounds the three kinds together, no stream is added); every alternate
 * tracks in pyramids and track arrays of its own, allocated at its first Lucas-Kanade step.  want_arrays: the record carries
 * mask / q / xy (without it _end refuses them with VO_E_CAP).  Both slots may be refilled once _begin has returned: the refill orders
 * itself behind the step.  _end: VO_E_SWEEP as vo_pnp_pair_end; VO_E_STATE for a ticket of another kind -- and vo_pose_pair_end,
 * vo_pnp_pair_end and vo_pnp_pair_end_lo refuse a ticket of this kind with VO_E_STATE; a refused ticket stays open. */
int vo_klt_pnp_pair(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int klt_iters, double eps, double min_eig, double fb,
                    const double* K4, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds, int32_t* counts4, int32_t* flags,
                    double* Rt12, double* Rt12_refined, int32_t* refine2, int32_t* lo2, uint8_t* mask_out /*cap*/, int32_t* q_idx /*cap*/,
                    float* xy_out /*cap*2*/, int cap);
int vo_klt_pnp_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int klt_iters, double eps, double min_eig, double fb,
                          const double* K4, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds, int want_arrays, int* ticket_out);
int vo_klt_pnp_pair_end(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                        int32_t* lo2, uint8_t* mask_out /*cap*/, int32_t* q_idx /*cap*/, float* xy_out /*cap*2*/, int cap);

/* Dense direct alignment (an extension, NOT part of the reference): photometric refinement of the motion between two slots on the
 * dense disparity of the older one.  Slot a holds a dense disparity and its rectified left image (the TEMPLATE), slot b a rectified
 * left image of the same size; Rt0 is the initial a -> b motion in the PnP step's convention (X' = R X + t, X in frame a, pixel in b),
 * K4 = {fx, fy, cx, cy} in full-image pixels, as vo_pnp_pair takes it.  Defined by this build, operation by operation
 * (tests/direct_ref.py restates it): integer stages are exact, everything else is float64 in the order written below, every product
 * and sum rounded on its own (no fused multiply-add); only the ORDER of the sums over the points is the kernel's own (per thread
 * ascending, a tree over the wave, the waves in order), so the float64 results agree with the restatement to rounding, not in bits.
 *   Parameters: levels 1 .. VO_DIRECT_MAX_LEVELS, iters 1 .. 20, max_points >= 1, grad_min 0 .. 255 (an integer), huber > 0,
 *   0 < dmin <= dmax, z_min >= 0, min_pixels >= 6, all finite; Rt0 and K4 finite, fx, fy > 0.
 *   Pyramid: vo_klt_track's, of both left images: levels 0 .. levels - 1, level l of size (w_l, h_l); level-l pixel (x, y) stands for
 *   level-0 pixel (x 2^l, y 2^l); the level intrinsics are fx_l = fx / 2^l, fy_l, cx_l = cx / 2^l, cy_l (no half-pixel terms).
 *   Rectangle of level l: [x_lo, x_hi) x [y_lo, y_hi) = the level image, or with a ROI (vo_set_roi, clipped to the image) x_lo =
 *   ceil(x0 / 2^l), x_hi = floor(x1 / 2^l), and likewise in y.
 *   Lattice of level l: x = x_lo + 1 + i s < x_hi - 1 (i = 0 .. nx - 1), y = y_lo + 1 + j s < y_hi - 1 (j = 0 .. ny - 1), s the smallest
 *   positive integer with nx ny <= max_points (computed by the host, reported); the linear index of a point is j nx + i.
 *   Selection (integer, independent of the pose), A = level l of slot a's image: d16 = disp16_a[y 2^l][x 2^l] with 16 dmin <= d16 <=
 *   16 dmax; gx2 = A[y][x + 1] - A[y][x - 1], gy2 = A[y + 1][x] - A[y - 1][x] with gx2 gx2 + gy2 gy2 >= 4 grad_min grad_min.
 *   The 3-D point, from the Q of vo_set_Q: d = d16 / 16, W = Q[3][2] d + Q[3][3], X = (x 2^l + Q[0][3]) / W, Y = (y 2^l + Q[1][3]) / W,
 *   Z = Q[2][3] / W.
 *   One iteration at the pose Rt = [R | t] (row-major 3 x 4), for every selected point:
 *     x' = ((R00 X + R01 Y) + R02 Z) + t0, y', z' likewise; u = (fx_l x') / z' + cx_l, v = (fy_l y') / z' + cy_l;
 *     the point TAKES PART iff z' > z_min and x_lo <= u < x_hi - 1 and y_lo <= v < y_hi - 1;
 *     iu = floor(u), ax = u - iu, iv, ay likewise; b00 = B[iv][iu], b01 = B[iv][iu + 1], b10 = B[iv + 1][iu], b11 = B[iv + 1][iu + 1];
 *     I_b = (b00 (1 - ax) + b01 ax) (1 - ay) + (b10 (1 - ax) + b11 ax) ay;  r = I_b - A[y][x];  w = 1 for |r| <= huber, else huber / |r|;
 *     gx = gx2 / 2, gy = gy2 / 2 (the TEMPLATE's gradient);  a = ((gx fx_l) / z', (gy fy_l) / z', -(((gx fx_l) x' + (gy fy_l) y') / (z' z')));
 *     j = [X' x a | a] = (y' a2 - z' a1, z' a0 - x' a2, x' a1 - y' a0, a0, a1, a2): the component order of the PnP refit;
 *     sums: H[k] += (w j[p]) j[q] over p <= q in packed row order (21), g[p] += (w j[p]) r (6), count += 1, wr2 += (w r) r.
 *   Then H d = -g by the Cholesky step of the PnP refit and Rt <- [Exp(d[0..2]) R | Exp(d[0..2]) t + d[3..5]], as the refit does.
 *   Schedule: levels levels - 1 .. 0, `iters` iterations each, no early exit.  An iteration with count < min_pixels stops the step
 *   with status 2 ("starved"); a sum or a new pose that is not finite, or a pivot that is not positive, stops it with status -1;
 *   in both cases the pose returned is that of the last completed iteration (Rt0 when none completed).  Status 0: all ran.
 *   The record: status, iterations completed (over all levels); per level its s, the number of selected points (0 for a level the
 *   step never reached) and count and wr2 of the level's first and of its last evaluated iteration (an iteration that stopped the
 *   step counts as evaluated); the final Rt; and the 21 + 6 sums, count and wr2 of the last COMPLETED iteration's linearisation
 *   (zeros when none completed): H is the information matrix of the pose up to the noise scale.
 * One launch of one workgroup (k_direct_align) behind the pyramid launches on the context's stream, ONE host synchronisation; the
 * pyramids live in the Lucas-Kanade workspace of the main match scratch.  With vo_enable_timing on, the pyramid launches are
 * bracketed under VO_T_ORB and the alignment under VO_T_POSE.
 *   VO_E_ARG: a bad slot or pointer, a parameter outside the ranges above, a non-finite Rt0 / K4.  VO_E_STATE: slot a without a pair
 *   or without a dense disparity, or with keypoints that carry depth (a sparse slot); slot b without a pair; two slots of different
 *   shapes; no vo_set_Q.  VO_E_SWEEP: slot a's disparity is undefined (as vo_pose_pair_end).  A refused call writes no record. */
#define VO_DIRECT_MAX_LEVELS 4
typedef struct vo_direct_level {
    int32_t s, selected, n_first, n_last;
    double wr2_first, wr2_last;
} vo_direct_level;
typedef struct vo_direct_rec {
    int32_t status, iters_done, levels, pad;
    vo_direct_level lv[VO_DIRECT_MAX_LEVELS];
    double Rt[12];
    double sums[27]; /* H (21, packed upper triangle in row order), g (6) */
    double count, wr2;
} vo_direct_rec;
int vo_direct_align(vo_ctx* ctx, int slot_a, int slot_b, const double* K4, const double* Rt0 /*12*/, int levels, int iters, int max_points,
                    int grad_min, double huber, double dmin, double dmax, double z_min, int min_pixels, vo_direct_rec* rec_out);

/* The dense direct alignment with an AFFINE BRIGHTNESS term: a gain k and an offset m of image B are estimated beside the pose, for
 * pairs whose exposure moved (vo_direct_align assumes brightness constancy).  Defined operation by operation like vo_direct_align
 * (tests/direct_ab_ref.py restates it); EVERYTHING through I_b is vo_direct_align's: pyramid, rectangle, lattice, selection, the 3-D
 * point, the test of taking part, the bilinear sample; so are the float64 rules (every product and sum rounded on its own) and the
 * order of the sums over the points.  What differs:
 *   State: (k, m) starts at (1, 0) and is carried over iterations AND levels (the brightness of a pair does not depend on the level).
 *   Residual: r = (k I_b + m) - A[y][x]; w = 1 for |r| <= huber, else huber / |r|, on this r.  The correction is applied to B so that
 *   the pose columns can stay the TEMPLATE's: at the solution k grad I_b = grad A.
 *   Columns: j[0..5] exactly vo_direct_align's; j[6] = I_b (dr / dk), j[7] = 1 (dr / dm).
 *   The iteration index within a level is it = 0 .. iters - 1.  it < 2: the iteration is HELD -- the 21 + 6 sums of j[0..5], count and
 *   wr2 with the r above, the 6 x 6 solve and the twist of vo_direct_align; (k, m) keep their values.  Otherwise it is FREE: H[k] +=
 *   (w j[p]) j[q] over p <= q < 8 in packed row order (36), g[p] += (w j[p]) r (8), count, wr2; H d = -g by the same Cholesky scheme
 *   on 8 unknowns; the twist from d[0..5] as ever; k <- k + d[6], m <- m + d[7].  (Why held iterations: against an image that is
 *   still misaligned the best linear brightness fit has a slope below 1, and a pose freed together with it settles there.)
 *   Parameters: iters 3 .. 20 (with fewer than three iterations none would be free); all other ranges are vo_direct_align's.
 *   Status: vo_direct_align's, and -1 also when the new k or m is not finite or the new k <= 0.  The new pose, k and m are committed
 *   together or not at all: the record returns those of the last completed iteration ((1, 0) and Rt0 when none completed).
 *   The record: vo_direct_align's fields; k, m; unknowns = 6 or 8, the size of the last COMPLETED iteration's linearisation (6 when
 *   none completed); sums = its H then its g: 36 + 8 for unknowns 8, 21 + 6 followed by zeros for unknowns 6; its count and wr2.
 * One launch of one workgroup (k_direct_align_ab), ONE host synchronisation, timing brackets and errors as vo_direct_align. */
typedef struct vo_direct_ab_rec {
    int32_t status, iters_done, levels, unknowns;
    vo_direct_level lv[VO_DIRECT_MAX_LEVELS];
    double Rt[12];
    double k, m;
    double sums[44]; /* H (packed upper triangle in row order), g: 36 + 8, or 21 + 6 and zeros */
    double count, wr2;
} vo_direct_ab_rec;
int vo_direct_align_ab(vo_ctx* ctx, int slot_a, int slot_b, const double* K4, const double* Rt0 /*12*/, int levels, int iters, int max_points,
                       int grad_min, double huber, double dmin, double dmax, double z_min, int min_pixels, vo_direct_ab_rec* rec_out);

/* PATCH ALIGNMENT (an extension, NOT part of the reference): the photometric refinement for SPARSE stereo depth -- sparse model-based
 * image alignment.  The points are small pixel patches around slot a's depth-carrying keypoints, every pixel of a patch sharing its
 * keypoint's depth; no disparity image is read.  Defined operation by operation like vo_direct_align (tests/direct_kp_ref.py restates
 * it); EVERYTHING not stated here is vo_direct_align's, word for word: the pyramid, the level intrinsics, the rectangle of a level with
 * and without a ROI, one iteration from x' on (the test of taking part, the bilinear sample, r, the Huber weight, the TEMPLATE's
 * gradient in the Jacobian, the 21 + 6 + 2 sums), the Cholesky solve and the twist, the schedule, the statuses 0 / 2 / -1, "the pose
 * of the last completed iteration", the float64 rules and the order of the sums over the points (per thread ascending in the point
 * index below, a tree over the wave, the waves in order).
 *   Inputs: slot a holds a pair and keypoints that carry depth (vo_sparse_stereo); n, kp_xy (pixels of the ROI crop) and the Z of
 *   kp_xyz are read, kp_disp is NOT.  Slot b holds a pair of the same shape; it needs no keypoints.  patch is 3, 5 or 7, hp = patch / 2
 *   (integer); all other parameter ranges are vo_direct_align's.  Q[2][3] must be finite and not zero.
 *   Keypoint i (x_i, y_i float32, Z_i float32): vx = (double)(x_i + (float)ox), vy = (double)(y_i + (float)oy), the additions in
 *   float32 as step d of vo_sparse_stereo, (ox, oy) the origin of the ROI crop ((0, 0) without a ROI).  The keypoint is USABLE iff
 *   vx, vy and Z_i are finite, Z_i > 0, 0 <= vx < w and 0 <= vy < h -- tested in floating point BEFORE any conversion to an integer.
 *   s_i = (double)Z_i / Q[2][3].
 *   Level l: cx = (int)rint(vx / 2^l), cy = (int)rint(vy / 2^l) (half to even).  A usable keypoint is IN USE at level l iff its patch
 *   and the one-pixel ring the gradient reads lie in the level's rectangle: cx - hp >= x_lo + 1, cx + hp <= x_hi - 2, cy - hp >= y_lo + 1,
 *   cy + hp <= y_hi - 2.  Its points: (x, y) = (cx + dx, cy + dy) for dx, dy = -hp .. hp, point index i patch^2 + (dy + hp) patch +
 *   (dx + hp).  Overlapping patches and duplicate keypoints each contribute: nothing is de-duplicated.
 *   Selection: gx2 = A[y][x + 1] - A[y][x - 1], gy2 = A[y + 1][x] - A[y - 1][x] with gx2 gx2 + gy2 gy2 >= 4 grad_min grad_min.
 *   The 3-D point: X = (x 2^l + Q[0][3]) s_i, Y = (y 2^l + Q[1][3]) s_i, Z = (double)Z_i.
 *   The record: vo_direct_rec; lv[l].s = the number of keypoints in use at level l (0 for a level the step never reached), pad = patch;
 *   everything else as vo_direct_align fills it.
 * One launch of one workgroup (k_direct_align_kp) behind the pyramid launches, ONE host synchronisation, the timing brackets of
 * vo_direct_align.
 *   VO_E_ARG: a bad slot or pointer, a parameter outside its range (patch other than 3, 5, 7), a non-finite Rt0 / K4.  VO_E_STATE:
 *   a slot without a pair; slot a's keypoints carry no depth (a dense slot, or none extracted); two slots of different shapes; no
 *   vo_set_Q, or a Q[2][3] that is zero or not finite.  VO_E_CAP: slot a holds more keypoints than the context's capacity, or
 *   n patch^2 does not fit the 31-bit point index.  A refused call writes no record. */
int vo_direct_align_kp(vo_ctx* ctx, int slot_a, int slot_b, const double* K4, const double* Rt0 /*12*/, int levels, int iters, int patch,
                       int grad_min, double huber, double z_min, int min_pixels, vo_direct_rec* rec_out);

/* instrumentation ------------------------------------------------------------------------ */
/* hipEvent timing of the kernels launched on the context stream (events are recorded without
 * blocking and resolved by vo_get_timings).  Stage ids: */
enum { VO_T_UPLOAD = 0, VO_T_SGBM_COST, VO_T_SGBM_AGG, VO_T_SGBM_WTA, VO_T_SGBM_POST, VO_T_ORB,
       VO_T_MATCH, VO_T_POSE, VO_T_KNN /* the Hamming kNN kernel alone (inside VO_T_MATCH or VO_T_POSE) */, VO_T_NSTAGES };
/* on = 0 off, 1 every stage, otherwise (stage bit mask << 1), e.g. (1 << VO_T_SGBM_AGG) << 1 */
int vo_enable_timing(vo_ctx* ctx, int on);
/* accumulated milliseconds and launch counts per stage since the last reset */
int vo_get_timings(vo_ctx* ctx, double* ms_out /*VO_T_NSTAGES*/, int64_t* launches_out, int reset);
/* Development aid: the brackets recorded since vo_get_timings last resolved them, one by one and in the order they were opened
 * -- stage id, entries (pairs a sweep group's launch carries), begin and end in milliseconds relative to the begin of the first
 * of them (brackets lie on different streams: a begin may be negative).  Waits for every stream of the context, writes at most
 * `cap` brackets, *n_out = how many there are; a bracket whose events cannot be resolved is left out.  Consumes nothing (a
 * following vo_get_timings accumulates the same brackets); *n_out = 0 while timing is off. */
int vo_get_stage_timeline(vo_ctx* ctx, int cap, int32_t* stage_out, int32_t* entries_out, double* begin_ms_out, double* end_ms_out, int* n_out);
/* algorithmic cost-volume cells (width1*H*D) of the last vo_sgbm_compute, and the number of path directions its dominant
 * aggregation kernel covers (3: NW / N / NE inside k_sgbm_diag; 1 in mode 2: N inside k_sgbm_vert; all of them -- 5, 8 or,
 * in mode 2, 3 -- for uniquenessRatio >= 100) */
int vo_sgbm_last_geometry(vo_ctx* ctx, int64_t* cells, int* n_paths);
/* which aggregation schedule the latest SGBM run of this context took -- it follows from the parameters alone (every
 * schedule gives the same bits: stereo_camera.py:51 only sees the disparity) */
enum { VO_SCHED_DIAG = 1,          /* W + E as one volume (k_sgbm_we), NW / N / NE + WTA in the diagonal sweep */
       VO_SCHED_DIAG_RAGGED = 2,   /* the same with k_sgbm_pair for W + E (width - numDisparities not a multiple of 8) */
       VO_SCHED_UNFUSED = 3,       /* uniquenessRatio >= 100: one volume per direction + per-pixel winner search */
       VO_SCHED_VERT = 4,          /* mode 2: W + E as one volume (k_sgbm_we2 / k_sgbm_we), N + WTA in the vertical sweep (k_sgbm_vert) */
       VO_SCHED_VERT_RAGGED = 5 }; /* the same with k_sgbm_pair for W + E */
int vo_sgbm_last_schedule(vo_ctx* ctx, int* schedule_out);
/* measurement aid (SURVEY 8(d) "device-copy ceiling"): `reps` streaming copies of `bytes` (<= one cost volume; 0 = a
 * whole one) between two of the context's volumes, timed with HIP events; *gb_per_s counts bytes read + bytes written.
 * Overwrites the cost volume: call it between, not inside, vo_sgbm_compute / vo_prefetch_pair sequences. */
int vo_measure_copy(vo_ctx* ctx, int64_t bytes, int reps, int nontemporal, double* gb_per_s);
/* Measurement aid: `reps` launches of the Hamming kNN-2 kernel (slot_a's descriptors against slot_b's) back to back on the main
 * stream between two HIP events -> microseconds per launch (the event pair's own cost is spread over the launches).  The result
 * arrays are the context's match scratch; nothing the caller holds changes.  Semantics of the kernel: stereo_odometer.py:163. */
int vo_measure_knn(vo_ctx* ctx, int slot_a, int slot_b, int reps, double* us_per_launch);
/* the same for either form of the kernel: match_flags 0 = the plain kNN-2, VO_MATCH_CROSSCHECK = kNN-2 + column minima (and the
 * reset of the column words on the stream in front of each launch, which is part of what a cross-check launch costs),
 * VO_MATCH_WINDOW = inside the context's window around the two slots' keypoint positions */
int vo_measure_knn_ex(vo_ctx* ctx, int slot_a, int slot_b, int reps, int match_flags, double* us_per_launch);
/* the shader clock the GPU holds right now (MHz): one wave counts its cycles (s_memtime) against the 100 MHz wall counter
 * (s_memrealtime) for `micros` microseconds on the context's main stream; synchronous.  Measurement aid (bench.py records it
 * after every timed window: a GPU that has been idle ramps its clock up over the first tens of milliseconds of work). */
int vo_shader_clock(vo_ctx* ctx, int micros, double* mhz);
/* health of the diagonal aggregation sweeps (synchronises): *error_out = number of SGBM runs of this context in which a wait
 * between strips exceeded its poll limit (the affected pair's results are refused with VO_E_SWEEP where they are picked up:
 * vo_sgbm_compute with an output pointer, vo_download_disparity_f32 / _xyz, vo_orb_detect_and_compute with the fused mask,
 * vo_points3d_at, vo_point_clouds, vo_pose_pair, vo_pose_pair_end, vo_pnp_pair, vo_pnp_pair_end); the count is sticky until vo_destroy, a later pair in
 * the same workspace is unaffected */
int vo_sgbm_sweep_status(vo_ctx* ctx, int* error_out);
/* development aid: control block `block` (0 | 1) of the latest aggregation sweep in the main workspace -- word 0 = work items
   taken, word 1 = a wait gave up in this launch (cleared by the next run), words 8 + 8 s .. = {start, end, failed polls, ticks waiting, misses} of strip s (100 MHz ticks).
   No reference counterpart (stereosgbm.cpp is one sequential pass). */
int vo_sgbm_sweep_stats(vo_ctx* ctx, int block, int32_t* out, int n_words);

/* multi-GPU ----------------------------------------------------------------------------
 * NOT part of the reference (openVO is one process on one thread): frame pairs shard across the GPUs of a
 * node, one process per GPU, each running its own context on a contiguous chunk of the stream; the path's
 * only exchange is the gather of the relative poses -- 17 float64 per frame: the row-major 4x4 transform
 * one accepted update() multiplied into c_T_w [stereo_odometer.py:137-138,146-149] and the accept flag --
 * done with RCCL (ncclAllGather over xGMI), bound directly: librccl.so.1 is loaded on first use.  Rank 0
 * obtains the 128-byte id with vo_mgpu_unique_id and hands it to the other ranks by any means (the Python
 * host uses a TCP socket on the node); every rank then calls vo_mgpu_create with the same id. */
typedef struct vo_mgpu vo_mgpu;
int vo_device_count(int* n_out);                       /* HIP devices visible to this process (0 if none) */
int vo_mgpu_unique_id(uint8_t* id128 /*128 bytes*/);   /* ncclGetUniqueId */
int vo_mgpu_create(int device, int rank, int world, const uint8_t* id128, vo_mgpu** out);   /* ncclCommInitRank */
void vo_mgpu_destroy(vo_mgpu* g);
/* what RCCL itself reports for the communicator: ncclCommCount, ncclCommUserRank, and the device it was created on */
int vo_mgpu_info(vo_mgpu* g, int* n_ranks, int* user_rank, int* device);
const char* vo_mgpu_last_error(const vo_mgpu* g);      /* g may be NULL: error of the last failed create / id call */
/* every rank passes n_frames x 17 float64 (same n_frames on every rank); all_n17 receives world x n_frames x 17
 * in rank order */
int vo_mgpu_gather_poses(vo_mgpu* g, const double* local_n17, int n_frames, double* all_n17);
int vo_mgpu_all_gather_f64(vo_mgpu* g, const double* local, int n, double* all /*world*n*/);
/* element-wise max over the ranks, in place (the slowest rank's time of a benchmark; doubles as a barrier) */
int vo_mgpu_all_reduce_max_f64(vo_mgpu* g, double* v, int n);

#ifdef __cplusplus
}
#endif
#endif
