// Internal declarations of libvo355 (gfx950 only).  See include/vo355.h for the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <deque>
#include <thread>
#include <mutex>
#include <condition_variable>
#include "../../include/vo355.h"
#include "ransac_ws.h"

#define VO_ORB_LEVELS 8
#define VO_ORB_EDGE 31
#define VO_ORB_HALF_PATCH 15

struct SgbmEff {
    int minD, maxD, D, ur, d12, P1, P2, SW2, SH2, ftzero, minX1, maxX1, W1, invalid16;
    int speckleWindow, speckleRange, mode;
    bool set;
};

struct OrbLevel {
    int w, h;            // level size
    size_t off;          // byte offset of the level inside the pyramid buffers
    float scale;         // 1.2^l as float
    int quota;           // filled per call (depends on nfeatures)
};

struct FrameSlot {
    uint8_t* left = nullptr;    // rectified gray, max_w*max_h
    uint8_t* right = nullptr;
    int16_t* disp16 = nullptr;  // max_w*max_h
    // keypoints (device), capacity kp_cap
    float* kp_xy = nullptr;
    float* kp_size = nullptr;
    float* kp_angle = nullptr;
    float* kp_resp = nullptr;
    int32_t* kp_oct = nullptr;
    uint8_t* desc = nullptr;
    int n_kp = 0;
    int w = 0, h = 0;
    bool has_pair = false, has_disp = false, has_kp = false;
    // look-ahead: the pair was ingested + SGBM'd on the second stream; `ready` orders consumers
    hipEvent_t ready = nullptr;
    bool pending = false;
    bool counted = false;        // part of vo_lookahead_depth (submitted, neither waited for nor dropped)
    // asynchronous pose steps still reading this slot on their own streams (vo_pose_pair_begin): whoever overwrites the slot
    // orders itself behind them (borrowed events: they belong to the pose alternates and live as long as the context)
    hipEvent_t readers[2] = {nullptr, nullptr};
    // monocular pose steps (vo_mono_pose_pair): depth of each keypoint along the optical axis, in units of the baseline of the step
    // that wrote it (0 = none), kp_cap doubles; [0] of mono_serial_dev is that step's serial, stamped by its last kernel.  mono_serial
    // is the host's copy: set when the step is enqueued, cleared by whatever refills the slot or re-extracts its keypoints (the
    // device word may then be stale: a step is only ever handed depths whose serial the HOST copy still confirms).  depth_writer: the
    // `done` event of the asynchronous step that writes the array (borrowed like `readers`): a later step's tail waits for it.
    double* mono_depth = nullptr;
    uint32_t* mono_serial_dev = nullptr;
    uint32_t mono_serial = 0;
    hipEvent_t depth_writer = nullptr;
    // look-ahead ORB: keypoints were extracted behind the SGBM on the engine's stream; the count lands
    // in the slot's pinned word once `ready` has fired
    int32_t* n_kp_host = nullptr;
    bool kp_pending = false;
    // health of the disparity in this slot: every SGBM run gets a generation number (disp_gen, never 0); a run whose diagonal
    // sweep gave up a strip hand-off (its disparity is then undefined) writes ITS generation into the slot's pinned word from
    // the device (k_sgbm_fin).  The slot is bad exactly while *sweep_word == disp_gen: a refill gets a new generation, a late
    // write of an older run can never match it.  Checked wherever the host picks up results that depend on the disparity.
    int32_t* sweep_word = nullptr;
    int32_t disp_gen = 0;
    int kp_params[4] = {0, 0, 0, 0};   // nfeatures, mask_mode, min_disp16, max_disp16 of the pending run
    // sparse stereo depth (vo_sparse_stereo): 3-D position (3 floats) and disparity of each keypoint, kp_cap entries.  kp_depth: the
    // keypoints the slot holds carry them (and are only the keypoints that have a depth); cleared by every ORB extraction into the
    // slot and by every refill.  The pose steps read their points from kp_xyz when BOTH slots' keypoints carry depth.
    float* kp_xyz = nullptr;
    float* kp_disp = nullptr;
    bool kp_depth = false;
    // ... and the descriptor (32 bytes) of the RIGHT keypoint each of them was associated with: valid exactly while kp_depth is
    // (its x is the keypoint's x - kp_disp); the loop check of the pair steps reads it
    uint8_t* kp_rdesc = nullptr;
    // sparse stereo begun ahead (vo_prefetch_*_sparse): the whole chain was enqueued on a look-ahead engine's stream with the request
    // sp_req, and the slot's pinned record sp_rec = {left keypoints, accepted, kept, right keypoints} (the two extractions' counts as
    // they left them, unclamped) is written by its last kernel; vo_sparse_stereo with the same request only waits for `ready` and
    // reads the record.  sp_pending is cleared like kp_depth: by every ORB extraction into the slot and by every refill.  sp_req
    // stays that of the result the slot holds while kp_depth is set (a repeated call returns the record's counts again).
    int32_t* sp_rec = nullptr;
    bool sp_pending = false;
    bool sp_ahead = false;       // the sparse result the slot holds was begun ahead and has been collected: the same request again returns its counts
                                 // (never set by a synchronous computation, which always recomputes; voided by vo_set_Q / vo_set_roi)
    // assoc_flags / assoc_ratio: the association tests in force when the chain was enqueued (vo_set_sparse_assoc): part of the request
    struct SparseReq { int nfeatures; float min_disp, max_disp, row_tol; int max_hamming; int assoc_flags; float assoc_ratio; } sp_req = {-1, 0.f, 0.f, 0.f, 0, 0, 0.f};
    // the slot's look-ahead run is a member of the context's open sweep group: its diagonal sweep, post filters and ORB chain are
    // not enqueued and `ready` is NOT recorded for this run yet -- whoever is about to wait on, read, refill or drop the slot
    // closes the group first (sweep_group_close_for)
    bool in_group = false;
};

// scratch of one ORB run (pyramids, candidate lists, counters); one per look-ahead engine
struct OrbWs {
    uint8_t *pyr_img = nullptr, *pyr_mask = nullptr;
    int32_t *cand_pos = nullptr, *candA_pos = nullptr, *candB_pos = nullptr, *counters = nullptr;
    float *cand_resp = nullptr, *candA_resp = nullptr, *candB_resp = nullptr;
    hipEvent_t done = nullptr;   // end of the latest run in this workspace (any stream)
    bool done_valid = false;
};

// Scratch of one sparse stereo chain (sparse.hip): the two extractions' keypoint sets, each with its pinned count word (keypoint
// arrays and n_kp_host of a FrameSlot, nothing else), the ORB scratch of the second extraction (the first runs in the scratch the
// context works in: *ctx->orbws), per left keypoint the associated right keypoint (-1: none), the refined disparity (NaN: rejected)
// and its 3-D position, the ticket word of k_sparse_pair (zero between launches) and one claim word per right keypoint for the mutual
// test (0xFFFFFFFF between launches: set once by sparse_ws_prepare, put back by the launch that used them).  The context owns one for its main stream
// (l / r: the scratch slot of the *_host seams and sparse_r) and one per look-ahead engine, each completed at its first sparse use
// (sparse_ws_prepare) and freed by vo_destroy.
struct SparseWs {
    FrameSlot *l = nullptr, *r = nullptr;
    OrbWs orb_r;
    int32_t* match = nullptr;
    float *disp = nullptr, *xyz = nullptr;
    int32_t* ticket = nullptr;
    uint32_t* claim = nullptr;       // kp_cap words
    FrameSlot* own = nullptr;        // an engine's two sets (the main one borrows the context's)
    int32_t* own_words = nullptr;    // ... and their pinned count words
    bool ready = false, orb_ready = false;
};
typedef FrameSlot::SparseReq SparseReq;

// Landmark map (map.hip; include/vo355.h, vo_map_*): one set of the per-landmark arrays, `capacity` entries each
struct MapSet {
    float* xyz = nullptr;                      // 3 floats, world coordinates
    uint8_t *desc = nullptr, *rdesc = nullptr; // 32 bytes each
    int32_t *oct = nullptr, *obs = nullptr, *last = nullptr;
};
// A map of a context.  set[cur] holds the n landmarks; an update compacts into set[cur ^ 1] and flips.  view_src[k] = the landmark
// keypoint k of the last view came from (view_n of them; 0 = no view: void after every update, reset and plant).  claimed: one byte
// per keypoint of the frame being folded in; d_q / d_t / d_mask: the device copies of the caller's match arrays (kp_cap entries
// each).  seen: the host's scratch of the duplicate check (kp_cap bytes).  Everything is allocated by vo_map_create.
struct LandmarkMap {
    bool used = false;
    int capacity = 0, n = 0, cur = 0, view_n = 0;
    int max_serial = -1;                       // the largest serial an update has used since the last reset (-1: none)
    MapSet set[2];
    int32_t *view_src = nullptr, *d_q = nullptr, *d_t = nullptr;
    uint8_t *claimed = nullptr, *d_mask = nullptr;
    uint8_t* d_track = nullptr;                // the device block of vo_track_map (MapTrackDev: what its kernels hand each other)
    std::vector<uint8_t> seen;
};
void map_free(LandmarkMap& m);

// Lucas-Kanade tracking (klt.hip; include/vo355.h, vo_klt_*): the two pyramids of a call -- image 0 / 1, level l at byte off[l] of
// pyr[k], laid out for max_w x max_h (level 0 is only used by the host entry: the slot entry reads the slots' own images) -- and the
// per-point arrays, kp_cap entries each.  A member of a match workspace (vo_ctx::MatchWs::klt): the context's main one serves
// vo_klt_track / vo_klt_track_host / vo_klt_pnp_pair, a pose alternate's its own vo_klt_pnp_pair_begin step, so two steps in flight
// never share pyramids or track arrays.  Allocated at the first Lucas-Kanade use of that workspace, freed with it (match_ws_free).
#define VO_KLT_MAX_LEVELS 6
struct KltWs {
    uint8_t* pyr[2] = {nullptr, nullptr};
    size_t off[VO_KLT_MAX_LEVELS] = {};
    float *xy_in = nullptr, *xy_out = nullptr;
    uint8_t* status = nullptr;
    int32_t* iters = nullptr;
    bool ready = false;
};
void klt_ws_free(KltWs& k);
struct vo_ctx;
// completes the Lucas-Kanade members of the match workspace in force at their first use (klt.hip): the caller of klt_pyr_enqueue does it
int klt_ws_prepare(vo_ctx* ctx);
// the pyramids above level 0 of two images of one size into that workspace (k_klt_pyr_down, one launch per level on ctx->stream);
// a / b / lw / lh receive VO_KLT_MAX_LEVELS entries each (klt.hip; used by direct.hip too)
int klt_pyr_enqueue(vo_ctx* ctx, const uint8_t* a0, const uint8_t* b0, int w, int h, int levels, const uint8_t** a, const uint8_t** b, int* lw, int* lh);

struct vo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool hyp5_ready = false;       // k_ransac_hyp5 may ask for its 100 KB of LDS: set at this context's first five-point launch
    // look-ahead engines (vo_prefetch_*): each has its own stream and staging; engine 0 shares the main
    // SGBM workspace, engines 1.. own an alternate one, so several pairs' SGBM can be in flight (one
    // pair's latency-bound kernels overlap another's bandwidth-bound ones)
    static const int MAX_ENGINES = 24;
    hipStream_t la_stream[MAX_ENGINES] = {};
    // Lane streams (DESIGN 4f'''): while the group size in force is above 1, every dense look-ahead submission that may defer goes on the open
    // group's lane instead of its engine's stream, the group's chain follows on the same lane, and consecutive groups alternate
    // between the two lanes -- group g + 1's fronts run beside group g's chain, and nothing of one group can queue up behind the
    // other's chain in a hardware queue the two share.  Created at vo_create where groups are in force from the start -- the
    // first streams behind the main one -- otherwise when a setter puts them in force; used by nothing else.  An engine
    // whose latest work lies on another stream than the one it is given work on now is ordered by ONE event (engine_enter).
    // lanes_on: VO_GROUP_LANES (0 = every engine keeps to its own stream, as before the lanes).  lane_next: the lane the next
    // new group takes (the one the group closed last did not use).
    hipStream_t lane[2] = {nullptr, nullptr};
    bool lanes_on = true;
    // front_batch: VO_GROUP_FRONTS.  F >= 2: a dense look-ahead run that becomes a member of the open group on a lane leaves its
    // planes and cost volume to the group as well, and F pending members' fronts (or however many are pending when the group
    // closes) go in one launch each (DESIGN 4f'''').  0 / 1: every run launches its own front, as before.
    int front_batch = 8;
    bool lane_used = false;          // the latest look-ahead submission went on a lane (a dense stream is running on the lanes)
    int lane_next = 0;
    int cur_engine = -1;
    // VO_STAGGER = K: a pair's early stages (cost volume, W + E) start only after those of the pair K places before it have finished
    // (an event wait on the engine's stream; default: 7/16 of the engines, 0 = off).  Keeps the pairs in flight spread over the stages
    // -- at most K of them in the early ones -- instead of all in the same one after a cold start: +2.5 % on a 20-pair burst,
    // +1.5 % in the steady state with 16 engines (K = 6..8: 6 and 7 are 1 % ahead of 8 on the burst, equal in the steady state;
    // K <= 4 costs throughput, K >= 12 changes nothing).
    int tune_stagger = -1;
    uint8_t* la_stage[MAX_ENGINES] = {};
    // One SGBM workspace: everything a disparity run writes.  The context owns one (`main_ws`: the main stream and look-ahead
    // engine 0 use it) and one per further engine; `ws` / `orbws` name the workspace and the ORB scratch the code in sgbm.hip /
    // orb.hip works in right now -- the main ones, or an engine's while that engine is being fed (EngineScope).
    struct SgbmWs {
        uint32_t *planesL = nullptr, *planesR = nullptr;
        int16_t *C = nullptr, *S = nullptr, *disp_tmp = nullptr;
        int32_t *ccl_runlen = nullptr, *ccl_label = nullptr, *ccl_size = nullptr;
        int32_t* rec = nullptr;          // the diagonal sweep's winner records: two arrays of max_w * max_h + 64 words
        int S_vols = 0;
        uint64_t* sw_bnd = nullptr;
        size_t sw_bnd_bytes = 0;
        int* sw_ctl = nullptr;
        uint32_t sw_tag = 0;
        hipEvent_t done = nullptr;       // end of the latest SGBM run in this workspace (any stream)
        bool done_valid = false;
        bool done_on_engine0 = false;    // ... and look-ahead engine 0's stream is already ordered behind that record
        hipStream_t done_lane = nullptr; // ... which a sweep group left on this lane stream: work on that lane is behind it already
        bool ready = false;
        OrbWs orb;
        uint8_t* pinned = nullptr;       // host staging of vo_prefetch_pair (two raw images)
        hipEvent_t h2d_done = nullptr;   // the copies out of `pinned` have finished
        bool h2d_valid = false;
        hipEvent_t mid = nullptr;        // the early stages of the engine's latest pair have finished: cost volume and W + E, or -- a member
                                         // of a sweep group whose W + E travels with the group's launches -- the cost volume
        bool mid_valid = false;
        hipEvent_t swept = nullptr;      // the launches of the latest group this engine closed have finished (recorded behind the last of them)
        hipEvent_t chain = nullptr;      // borrowed: `swept` of the engine that closed the group this engine was last a non-closing member of,
                                         // until this engine's stream has been ordered behind it (engine_behind_chain); a later close on that
                                         // engine's stream re-records it later on the same stream, which only orders more
                                         // (per-engine streams only: with lanes the stream order and `moved` do all of this)
        hipStream_t on = nullptr;        // the lane stream that carries this engine's latest work (nullptr: the engine's own stream)
        hipEvent_t moved = nullptr;      // recorded on the stream the engine leaves when it is given work on another one (engine_enter)
    } ws_alt[MAX_ENGINES];           // [0]: only its ORB scratch / staging / events are used (engine 0 works in main_ws)
    SgbmWs main_ws;
    SgbmWs* ws = &main_ws;
    OrbWs* orbws = &main_ws.orb;
    // ORB behind the look-ahead SGBM (vo_set_lookahead_orb): nfeatures, mask_mode, min/max disp16
    bool la_orb = false;
    int la_orb_params[4] = {0, 0, 0, 0};
    int32_t* slot_words = nullptr;   // pinned: one word per slot (keypoint counts of pending runs), then one per slot for FrameSlot::sweep_word
    int32_t sweep_gen_next = 0;      // generations handed to SGBM runs so far
    int* d_sweep_errs = nullptr;     // device counter: SGBM runs of this context whose sweep gave up a hand-off (vo_sgbm_sweep_status)
    int tune_spin_limit = 1 << 22;   // polls before a wait inside the diagonal sweep is declared dead
    int fault_sweep = 0;             // VO_FAULT_SWEEP=n (VO_TEST_HOOKS builds only): the n-th diagonal sweep exports nothing and gives up after a few polls
    int engines_fit = 24;            // what 40 % of the device's free memory held at vo_create (vo_set_engines clamps to it)
    int n_engines = 16;              // VO_ENGINES (wants GPU_MAX_HW_QUEUES >= engines + 4: streams sharing a hardware queue serialise; with fewer the sweeps are grouped, see grp)
    int next_engine = 0;
    // Sweep groups (sgbm.hip): with fewer hardware queues than streams a pair's kernels queue up behind other pairs' on the same
    // queue, and the diagonal sweep -- a latency chain that keeps ~28 CUs busy for a millisecond -- is the longest of them.  The
    // look-ahead path then collects up to B pairs whose early stages are enqueued (the open group) and sweeps them in ONE launch,
    // with one launch of W + E before it and one of each post filter and of each kernel of the look-ahead ORB chain behind it
    // for all of them.
    // hw_queues: GPU_MAX_HW_QUEUES as the process sees it (unset: HIP's 4).  sweep_group_req: VO_SWEEP_GROUP / vo_set_sweep_group,
    // 0 = follow the queue budget (sweep_group_size).  grp_closed: groups closed so far, by cause (VO_GRP_*).
    int hw_queues = 4;
    int sweep_group_req = 0;
    struct SweepGroup* grp = nullptr;
    int64_t grp_closed[4] = {0, 0, 0, 0};
    int max_w = 0, max_h = 0, max_disp = 0, max_kp = 0, kp_cap = 0;
    std::string err;
    char devname[256] = {0};

    SgbmEff sg{};
    struct { int cost = 0, cw = 9, ch = 7; } sg_cost;       // vo_set_sgbm_cost: VO_SGBM_COST_*, the census window; outlives vo_set_sgbm
    struct { bool valid = false; int H = 0, W1 = 0, D = 0, Dp = 0; } c_last;   // C of the latest synchronous run in the main workspace (vo_sgbm_cost_volume)
    double Q[16];
    bool has_Q = false;
    int roi[4] = {0, 0, 0, 0};
    bool has_roi = false;

    // rectification maps
    int16_t* map1[2] = {nullptr, nullptr};
    uint16_t* map2[2] = {nullptr, nullptr};
    int map_w = 0, map_h = 0;
    bool has_map[2] = {false, false};

    FrameSlot slots[VO_NUM_SLOTS + 1];  // last slot = scratch for the *_host seams
    // vo_sparse_stereo: the left keypoints are extracted into the scratch slot above, the right ones into this second scratch set
    // (keypoint arrays and pinned count word only); sp_main: the SparseWs of the main stream built on the two, sp_alt[k]: look-ahead
    // engine k's own
    FrameSlot sparse_r;
    LandmarkMap maps[VO_NUM_MAPS];      // vo_map_create .. vo_map_destroy (freed by vo_destroy too)
    SparseWs sp_main;
    SparseWs sp_alt[MAX_ENGINES];

    // staging
    uint8_t* stage_in = nullptr;   // raw upload (max_w*max_h*3)
    size_t stage_bytes = 0;

    // SGBM workspace: see SgbmWs (ws->planesL: per pixel 2 x u32 (u,u0,u1 for both channels); ws->planesR: per pixel 6 x u32
    // pair-packed (v,v0,v1 x 2 channels); ws->C: cost volume; ws->S: aggregated volumes (S_vols of them); ws->disp_tmp: WTA output
    // before the LR check; ws->sw_bnd: boundary granules of the diagonal sweep (allocated on first use); ws->sw_ctl: its two control
    // blocks {work items taken, sticky error, ..., per-strip timeline}; ws->sw_tag: launches so far in that workspace)
    size_t vol_cells = 0;
    int16_t* dump = nullptr;       // sink for the stores of lanes past the end of their scan line
    int sw_ctl_words = 0;
    int tune_diag_wgs = 0;         // VO_DIAG_WGS (development): workgroups of one diagonal sweep (0 = one image row's worth of strips + 2)
    int tune_diag_dbg = 0;         // VO_DIAG_DEBUG (development): bit 0 / 1 = strips import / export nothing, 4 / 8 / 16 / 32 = skip the cost / W+E / diagonal / post stage
    int tune_diag_nwc = 0;         // VO_DIAG_WAVES: compute waves per strip workgroup (7, 11 or 15) for Dp <= 128; 0 = 7 for synchronous calls, 11 on the look-ahead engines (launch_diag)
    int64_t last_cells = 0;
    int last_paths = 0;
    int last_schedule = 0;         // VO_SCHED_* of the latest run (vo_sgbm_last_schedule)

    // ORB workspace
    OrbLevel lv[VO_ORB_LEVELS];
    int orb_w = 0, orb_h = 0;      // geometry the pyramid tables were built for
    size_t pyr_bytes = 0;
    int32_t* rs_ofs = nullptr;     // resize tables (all levels): x then y offsets
    uint16_t* rs_coef = nullptr;
    // k_orb_pyramid: the pyramid is cut into pyr_nbx x pyr_nby cones (one workgroup each); pyr_rects = per level the column
    // interval every cone column needs (own part + what the next level's interval reads), then the row intervals:
    // [l][bx][2] (inclusive lo, hi) for x, followed by [l][by][2] for y.  pyr_buf[2] = bytes of the largest even- / odd-level
    // rectangle (the kernel's two ping-pong LDS buffers per image kind).
    int32_t* pyr_rects = nullptr;
    int pyr_nbx = 0, pyr_nby = 0, pyr_buf[2] = {0, 0}, pyr_tab = 0;
    char rs_meta_host[1024];       // host copy of the level descriptors (LevelsDev)
    int orb_quota_nfeatures = -1;  // nfeatures the device quotas were uploaded for
    int cand_cap = 0;
    uint8_t* host_mask_dev = nullptr;  // explicit mask upload (scratch)

    // match / pose workspace.  MatchWs = what one matching + pose (or essential-matrix) step writes; the context owns one
    // (`main_mw`) and one per asynchronous alternate, `mw` names the one the code in match.hip / geom.hip / ransac.hip works in
    // right now (AltScope retargets it together with the stream; nothing is swapped member by member).  match_ws_alloc /
    // match_ws_free (match.hip) hold the one member / size table.
    struct MatchWs {
        int32_t *m_idx = nullptr, *m_count = nullptr, *m_dist = nullptr, *mq_idx = nullptr, *mt_idx = nullptr;   // m_count: match counter of the ratio filter
        float *pts_a = nullptr, *pts_b = nullptr, *xy_a = nullptr, *xy_b = nullptr;
        uint8_t *st_a = nullptr, *st_b = nullptr, *clique_ws = nullptr;
        size_t clique_ws_bytes = 0;
        uint8_t* ransac_ws = nullptr;    // grown on demand (ws_reserve), laid out per step (ransac_ws.h)
        size_t ransac_ws_bytes = 0;
        KltWs klt;                       // completed at the workspace's first Lucas-Kanade use (klt.hip)
    };
    MatchWs main_mw;
    MatchWs* mw = &main_mw;
    // the match window of VO_MATCH_WINDOW (vo_set_match_window): read when a step is ENQUEUED and handed to the kernel by value
    bool has_win = false;
    float win_rx = 0.f, win_ry = 0.f;
    // the loop check of VO_MATCH_LOOP (vo_set_match_loop): read when a step is ENQUEUED and handed to the kernel by value
    bool has_loop = false;
    int loop_max = 0;
    // the association tests of the sparse stereo chain (vo_set_sparse_assoc): read when a chain is ENQUEUED, kept in the slot's request
    int sp_assoc_flags = 0;
    float sp_assoc_ratio = 0.f;
    uint8_t* mq = nullptr;
    uint8_t* mt = nullptr;
    double* red = nullptr;         // reduction scratch
    // Asynchronous steps (vo_pose_pair_begin / _end, vo_mono_pair_begin / _end): an alternate = a match scratch of its own, a
    // stream, a pinned result record and a completion event; a ticket is an alternate's index.  One mechanism (alt_open /
    // AltScope / alt_close / alt_ticket / alt_wait in match.hip) serves both kinds.  What differs between them:
    //   * the pose alternates run on n_pose_streams streams they SHARE and do not own (alternate k on stream k % n): a context
    //     must stay at about twenty HIP streams (16 engines + main + these) -- beyond that the hardware queues are time-sliced
    //     in ~10 ms quanta and a pair's diagonal sweep stalls behind a descheduled neighbour (measured: 23 streams -> 200-1000
    //     pairs/s).  Steps that share a stream run back to back without the host in between; their scratch and records are
    //     separate.  Every monocular alternate owns its stream.
    //   * the pose alternates' scratch has the 3-D / clique members (MATCH_WS_POSE), the monocular ones' has not.
    //   * only the pose step depends on disparities: it remembers its slots and their generations for the health check at _end.
    struct AsyncAlt {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        uint8_t* result = nullptr;     // pinned record the step's last kernel writes (pose: PoseOut or PnpRec + arrays; monocular: see MONO_HDR)
        bool ready = false, busy = false;
        MatchWs mw;
    };
    enum { ALT_POSE = 0, ALT_MONO = 1 };
    static const int N_POSE_ALT = VO_NUM_POSE_ASYNC;
    static const int N_POSE_STREAMS = 3;
    int n_pose_streams = N_POSE_STREAMS;     // VO_POSE_STREAMS (1..3): fewer when the GPU's hardware queues are shared with other processes
    // While dense pairs travel on the lanes, a pose step parked on a slot's `ready` event holds back everything behind it in
    // its hardware queue: on a queue it shares with a lane that is the lane's next fronts, until the OTHER lane's chain is over.
    // Without VO_POSE_STREAMS in the environment the steps then keep to what the queue budget leaves beside the main stream and
    // the two lanes (hw_queues - 3, at least one: ONE stream with four queues) -- pose_stream_count, asked when a step is begun.
    bool pose_streams_env = false;
    hipStream_t pose_streams[N_POSE_STREAMS] = {};
    struct PoseAlt : AsyncAlt {
        int slot_a = -1, slot_b = -1;
        int32_t gen_a = 0, gen_b = 0;      // disparity generations of the two slots when the step was begun (slot health at _end)
        bool pnp = false, want = false;    // a vo_pnp_pair_begin step (its record is a PnpRec) / whose record carries mask, q, t
        int nq = 0;                        // query keypoints of that step
        int lo = 0;                        // its lo_rounds (vo_pnp_pair_begin_lo; 0: the plain step)
        bool klt = false;                  // a vo_klt_pnp_pair_begin step (a PnpRec too; its arrays are mask, q, t and the tracked xy)
    } pose_alt[N_POSE_ALT];
    static const int N_MONO_ALT = VO_NUM_MONO_ASYNC;
    struct MonoAlt : AsyncAlt {
        bool want = false;                 // the record carries mask / q / t / xy of the second frame behind its header
        bool pose = false;                 // a vo_mono_pose_pair_begin step: the record is a vo_mono_pose (ended by vo_mono_pose_pair_end)
        int nq = 0, nb = 0, min_n = 0;
    } mono_alt[N_MONO_ALT];
    int alt_next[2] = {0, 0};              // round-robin position per kind
    uint32_t mono_serial_next = 0;         // serials handed to monocular pose steps so far (never 0: FrameSlot::mono_serial)
    AsyncAlt& alt(int kind, int k) { return kind == ALT_POSE ? static_cast<AsyncAlt&>(pose_alt[k]) : mono_alt[k]; }
    static int alt_count(int kind) { return kind == ALT_POSE ? N_POSE_ALT : N_MONO_ALT; }
    std::vector<const void*> big_lds;      // kernels this context has allowed more than 64 KB of dynamic LDS (lds_allow_big)
    float* img3_ws = nullptr;
    size_t img3_ws_bytes = 0;
    void* pinned = nullptr;        // pinned host buffer: first 4 KB scalar readbacks, rest = transfer arena
    size_t pinned_bytes = 0;
    size_t arena_off = 0;          // bump pointer into the arena (reset by xfer_flush)
    struct PendingCopy { void* dst; const void* src; size_t bytes; };
    std::vector<PendingCopy> pending;  // device->host copies staged in the arena, scattered at flush

    // pinned staging buffers for host images filled AHEAD by a helper thread of the caller (vo_host_stage_pair) and consumed by
    // vo_prefetch_host_staged on the thread that drives the context: the launching thread does no memcpy
    static const int N_HOST_STAGE = VO_NUM_HOST_STAGE;
    // `state` (under stage_mu): 0 = idle or filled, 1 = a copy into the buffer is queued or running on the library's staging
    // thread, < 0 = that copy failed (VO_E_*).  `valid` / `h2d_done` are written by the driving thread (the upload out of
    // the buffer has been enqueued) and read by the staging thread before it overwrites the buffer: under stage_mu too.
    struct HostStage { uint8_t* pinned = nullptr; hipEvent_t h2d_done = nullptr; bool valid = false; int state = 0; } host_stage[VO_NUM_HOST_STAGE];
    // vo_host_stage_begin: the copy of a host pair into pinned memory runs on ONE thread owned by the library (started on first
    // use, joined by vo_destroy), so that a driving thread written in an interpreted language never shares its interpreter
    // lock with a copying thread
    struct StageJob { int buf; const uint8_t *left, *right; size_t per; };
    std::thread stage_thread;
    std::mutex stage_mu;
    std::condition_variable stage_cv;
    std::deque<StageJob> stage_jobs;
    bool stage_stop = false;

    // inputs staged in HBM
    uint8_t* staged = nullptr;
    int staged_n = 0, staged_w = 0, staged_h = 0, staged_ch = 1;

    // tuning knobs (environment), read once in vo_create and never written afterwards
    int tune_sweep_ty = 30;         // VO_SWEEP_TY: rows per tile of the cost sweep
    int mono_engine = 0;            // round robin of vo_prefetch_staged_mono
    int inflight = 0;               // look-ahead pairs submitted and not yet waited for (vo_lookahead_depth)
    int fault_pnp_range = 0;        // VO_FAULT_PNP_RANGE=n (VO_TEST_HOOKS builds only): the n-th PnP pair step holds its match indices to a train set of ONE descriptor (flag bit 1, VO_E_STATE)
    int fault_map_nan = 0;          // VO_FAULT_MAP_NAN=n (VO_TEST_HOOKS builds only): the n-th vo_track_map hands its decision kernel a pose with one NaN entry (decision 5: no planted input reaches it, the PnP step returns zeros where it has no pose)
    int fault_prefetch = 0;         // VO_FAULT_PREFETCH=n (VO_TEST_HOOKS builds only): the n-th look-ahead submission fails inside its engine scope

    // timing
    bool timing = false;
    unsigned timing_mask = ~0u;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_stage;
    std::vector<int> ev_entries;   // launches' worth of work per bracket (StageTimer)
    size_t ev_used = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double t_ms[VO_T_NSTAGES] = {0};
    int64_t t_n[VO_T_NSTAGES] = {0};
};

int vo_fail(vo_ctx* ctx, int code, const char* fmt, ...);
#define VO_HIP(ctx, call)                                                               \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess)                                                          \
            return vo_fail(ctx, VO_E_HIP, "%s failed: %s (%s:%d)", #call,              \
                           hipGetErrorString(e__), __FILE__, __LINE__);                 \
    } while (0)

#define VO_CHECK_LAUNCH(ctx) VO_HIP(ctx, hipGetLastError())

// hipEvent pair around a stage, recorded on the context stream WITHOUT blocking it; the pairs are
// resolved in vo_get_timings.
// `entries`: how many launches' worth of work the bracket holds (a sweep group's one launch carries that many pairs: the
// stage's time / count stays a per-pair figure).
struct StageTimer {
    vo_ctx* c;
    int stage;
    long idx;
    StageTimer(vo_ctx* ctx, int s, int entries = 1);
    ~StageTimer();
};

static inline int div_up(int a, int b) { return (a + b - 1) / b; }

// Small host<->device transfers go through the pinned arena: asynchronous copies from / to
// pageable memory make the runtime pin and unpin the pages on every call (hundreds of
// microseconds each).  xfer_d2h defers the final host memcpy to xfer_flush (which synchronises).
int xfer_h2d(vo_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int xfer_d2h(vo_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
int xfer_flush(vo_ctx* ctx);

// make the main stream wait for a slot whose look-ahead work may still be running
int slot_wait(vo_ctx* ctx, FrameSlot& f);
// the stream the context currently works on is about to overwrite the slot: order it behind work that still writes or reads it
int slot_before_overwrite(vo_ctx* ctx, FrameSlot& f);
// `done` marks the end of an asynchronous step that reads the slot: whoever overwrites the slot waits for it first
void slot_add_reader(FrameSlot& f, hipEvent_t done);
int orb_slot_enqueue(vo_ctx* ctx, FrameSlot& f, int nfeatures, int mask_mode, int min_disp16, int max_disp16);
// the same for n slots of one size (a sweep group's members) in ONE launch per kernel on ctx->stream, slot i through scratch ws[i]
int orb_slots_enqueue(vo_ctx* ctx, FrameSlot* const* f, OrbWs* const* ws, int n, int nfeatures, int mask_mode, int min_disp16, int max_disp16);
// one member of a batched extraction (orb_enqueue_jobs): where its keypoints go, its scratch, its source image and mask
struct OrbIn {
    FrameSlot* fs; OrbWs* ws;
    const uint8_t* img; const int16_t* disp16; const uint8_t* mask;
    int img_stride, disp_stride, mask_stride;
};
// n extractions of one geometry and one request on ctx->stream, one launch per kernel (enqueue only: the counts land in n_kp_host)
int orb_enqueue_jobs(vo_ctx* ctx, const OrbIn* in, int n, int w, int h, int nfeatures, int mask_mode, int min_d16, int max_d16);
// one extraction on ctx->stream into the keypoint arrays of *fs (enqueue only: the count lands in fs->n_kp_host)
int orb_enqueue(vo_ctx* ctx, FrameSlot* fs, const uint8_t* d_img, int img_stride, int w, int h, int nfeatures, int mask_mode,
                const int16_t* d_disp16, int disp_stride, int min_d16, int max_d16, const uint8_t* d_mask, int mask_stride);
// ---- sparse stereo (sparse.hip) ----
// VO_E_ARG / VO_E_CAP for a request no sparse entry accepts (nothing is enqueued before this has passed)
int sparse_req_check(vo_ctx* ctx, const SparseReq& q, const char* who);
// completes a SparseWs at its first use: the second ORB scratch, the per-keypoint arrays, an engine's keypoint sets, and the ticket,
// cleared on `stream` -- the stream that will use it -- and waited for
// with_orb = false: the host seam of the association alone (no extraction: no second ORB scratch)
int sparse_ws_prepare(vo_ctx* ctx, SparseWs& ws, hipStream_t stream, bool own_sets, bool with_orb = true);
// the one allocator of an ORB scratch (vo_ctx.hip)
int orb_ws_alloc(vo_ctx* ctx, OrbWs& o);
void orb_ws_free(OrbWs& o);
void sparse_ws_free(SparseWs& ws);
// ENQUEUES on ctx->stream: both extractions of the slot's pair as one batch of two, association + refinement + compaction into the
// slot's keypoint arrays, kp_xyz, kp_disp; the slot's record and n_kp_host are written by the last kernel.  No synchronisation
// -- with one exception: a crop with no pixel inside ORB's border (empty, or at most 62 pixels in either direction) has no keypoint;
// nothing is launched, the stream is WAITED for (an earlier run into the slot may still be writing the record) and the host clears
// the slot's record.  No scratch count word is ever written from the host: an engine's earlier pair may still be reading them.
int sparse_enqueue(vo_ctx* ctx, FrameSlot& f, SparseWs& ws, const SparseReq& q);
// the slot's keypoints carry depth (vo_sparse_stereo): the pose steps take their 3-D points from kp_xyz
static inline bool slot_sparse(const FrameSlot& f) { return f.has_kp && f.kp_depth; }
// kernel `fn` may use up to 160 KB of dynamic LDS: set once per context, before its first launch that needs more than 64 KB
int lds_allow_big(vo_ctx* ctx, const void* fn);
// Device memory that must read zero before its first use on WHATEVER stream: the context's streams are non-blocking, they do
// not synchronise with the null stream a plain memset runs on, and a memset landing in the middle of a launch clears state that
// launch has written (kNN tickets that have been drawn: the group's result is then never written).  So: cleared AND waited for.
static inline hipError_t dev_zero(void* p, size_t bytes)
{
    const hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
size_t pose_ws_bytes(int nq);
// transfer-arena space the caller hands to a kernel that writes host memory itself; given back by xfer_flush like every staging
// block (nullptr when the arena is full: flush first)
void* xfer_stage(vo_ctx* ctx, size_t bytes);

// float64 wave sum on DPP moves (two per step); every lane of the result is NOT valid -- lane 63 is, and it is broadcast
__device__ __forceinline__ double wave_sum_f64_dpp(double v)
{
#define DPP_ADD64(ctrl, rmask)                                                                             \
    {                                                                                                      \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, rmask, 0xf, false);         \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, rmask, 0xf, false);         \
        v += __hiloint2double(hi, lo);                                                                     \
    }
    DPP_ADD64(0x111, 0xf) DPP_ADD64(0x112, 0xf) DPP_ADD64(0x114, 0xf) DPP_ADD64(0x118, 0xf)
    DPP_ADD64(0x142, 0xa) DPP_ADD64(0x143, 0xc)
#undef DPP_ADD64
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
// CROSS: a match must also pass the cross-check (knn_mutual on the column words of the same kNN launch)
// rd_q / rd_t (both or neither) + loop_max: the loop check -- the right partners' descriptors of the two slots (kp_rdesc)
template <bool CROSS>
__global__ void k_ratio_compact(const int32_t* idx, const int32_t* dist, int nq, double ratio, const float* xy_q, const float* xy_t,
                                int32_t* q_out, int32_t* t_out, float* xyq_out, float* xyt_out, int32_t* m_out,
                                const uint32_t* colmin, int nt, const uint8_t* rd_q, const uint8_t* rd_t, int loop_max);   // pose / clique scratch for nq query keypoints

// implemented in the per-stage files
// f.left, f.right (w x h) -> f.disp16; gives the run its generation.  srcL / srcR (both or neither): the rectified gray pair lies
// THERE in device memory and f.left / f.right still have to receive their copy (done by the run's first kernel)
// `deferred` (look-ahead engines only): with a sweep group size above 1 the run may stop behind its early stages and join the
// open group instead (*deferred = true): the sweep, the post filters, the ORB chain and the slot's `ready` record then follow
// when the group closes.
int sgbm_run(vo_ctx* ctx, FrameSlot& f, int w, int h, const uint8_t* srcL = nullptr, const uint8_t* srcR = nullptr, bool* deferred = nullptr);
// ---- sweep groups (sgbm.hip) ----
enum { VO_GRP_FULL = 0, VO_GRP_CONSUMER = 1, VO_GRP_FLUSH = 2, VO_GRP_OTHER = 3 };
// the group size in force: the request if there is one, else 1 with a hardware queue per stream (GPU_MAX_HW_QUEUES >= engines
// + 4) and VO_SWEEP_GROUP_FEW_QUEUES without; never above the number of engines (an engine holds one member at a time)
// With lanes the automatic size is at most half the engines: two consecutive groups then use disjoint engines (two banks), and
// no front ever waits for the other lane's chain.
#define VO_SWEEP_GROUP_FEW_QUEUES 12
static inline int sweep_group_size(const vo_ctx* ctx)
{
    int few = VO_SWEEP_GROUP_FEW_QUEUES;
    if (ctx->lanes_on && few > ctx->n_engines / 2) few = ctx->n_engines >= 2 ? ctx->n_engines / 2 : 1;
    int b = ctx->sweep_group_req > 0 ? ctx->sweep_group_req : (ctx->hw_queues >= ctx->n_engines + 4 ? 1 : few);
    return b < ctx->n_engines ? b : ctx->n_engines;
}
// lane mode is in force exactly while groups are: with group size 1 every launch and stream is the per-engine one
static inline bool lane_mode(const vo_ctx* ctx) { return ctx->lanes_on && ctx->lane[0] && ctx->lane[1] && sweep_group_size(ctx) > 1; }
static inline int pose_stream_count(const vo_ctx* ctx)
{
    int n = ctx->n_pose_streams;
    if (!ctx->pose_streams_env && ctx->lane_used && lane_mode(ctx) && n > ctx->hw_queues - 3) n = ctx->hw_queues - 3 > 1 ? ctx->hw_queues - 3 : 1;
    return n;
}
static inline bool stream_is_lane(const vo_ctx* ctx, hipStream_t s) { return s && (s == ctx->lane[0] || s == ctx->lane[1]); }
// every stream look-ahead engines' work can lie on has drained: the engines' own and the two lanes
static inline hipError_t engine_streams_sync(const vo_ctx* ctx)
{
    for (int k = 0; k < 2; k++)
        if (ctx->lane[k]) { const hipError_t e = hipStreamSynchronize(ctx->lane[k]); if (e != hipSuccess) return e; }
    for (int k = 0; k < vo_ctx::MAX_ENGINES; k++)
        if (ctx->la_stream[k]) { const hipError_t e = hipStreamSynchronize(ctx->la_stream[k]); if (e != hipSuccess) return e; }
    return hipSuccess;
}
// The open group's members finish on the closing member's stream: W + E, the sweep, the post filters and the ORB chain as one
// launch per kernel for all of them, then every member's `ready` record.  No other member's stream receives anything: an engine
// orders itself behind the chain when it is next given work (engine_behind_chain).  Nothing to do without an open group.  On
// failure every member's slot is left holding nothing.
int sweep_group_close(vo_ctx* ctx, int why);
// the open group's pending fronts are launched now (what they read is about to change); wait: and have run on return
int sweep_group_flush_fronts(vo_ctx* ctx, bool wait);
int engine_behind_chain(vo_ctx* ctx, int engine);
// The engine is about to be given work on `target` (its own stream or a lane), inside its EngineScope: ctx->stream becomes
// `target`, and where the engine's latest work lies on another stream, that stream gets an event record and `target` one wait
// for it (host-side decision, no host wait).  Includes engine_behind_chain.
int engine_enter(vo_ctx* ctx, int engine, hipStream_t target);
// the stream a dense look-ahead submission on `engine` goes on now: the open group's lane (without one: the lane the next
// group will take) in lane mode for a run that may defer (MODE_SGBM, the fused schedule), the engine's own otherwise
hipStream_t dense_stream(const vo_ctx* ctx, int engine);
bool sweep_group_has_engine(const vo_ctx* ctx, int engine);
int sweep_group_members(const vo_ctx* ctx);
void sweep_group_free(vo_ctx* ctx);
static inline int sweep_group_close_for(vo_ctx* ctx, const FrameSlot& f) { return f.in_group ? sweep_group_close(ctx, VO_GRP_CONSUMER) : VO_OK; }
// VO_E_SWEEP when the disparity the slot holds comes from a run whose sweep gave up a hand-off.  Only meaningful once the host
// has waited for work that depends on that run (a stream or event synchronisation).
int slot_health(vo_ctx* ctx, const FrameSlot& f, int slot);
int orb_prepare_tables(vo_ctx* ctx, int w, int h);
int orb_run(vo_ctx* ctx, FrameSlot* fs, const uint8_t* d_img, int img_stride, int w, int h,
            int nfeatures, int mask_mode, const int16_t* d_disp16, int disp_stride, int min_d16,
            int max_d16, const uint8_t* d_mask, int mask_stride);
// the kNN kernel's scratch lives behind the distances in ONE allocation (MatchWs::m_dist): 2 distances per query, then up to
// VO_KNN_SPLITS partial (best, second) pairs per query, then one ticket word per 64 queries (zero between launches), then one
// column word per train descriptor (cross-check launches only: reset to 0xFFFFFFFF on the launching stream before each of them)
#define VO_KNN_SPLITS 16
static inline size_t match_dist_bytes(int kp_cap)
{
    const size_t capq = ((size_t)kp_cap + 63) & ~(size_t)63;
    return capq * 8 + (size_t)VO_KNN_SPLITS * capq * 8 + (capq / 64 + 1) * 4 + capq * 4 + 256;
}
// the column words: ((|q| - 2 q.t + 256) << 16) | query of the nearest query of each train descriptor, ties to the lower query
static inline uint32_t* match_colmin(int32_t* d_dist, int kp_cap)
{
    const size_t capq = ((size_t)kp_cap + 63) & ~(size_t)63;
    return (uint32_t*)((uint8_t*)d_dist + capq * 8 + (size_t)VO_KNN_SPLITS * capq * 8 + (capq / 64 + 1) * 4);
}
// query i with nearest train t passes the cross-check iff t is a train index (checked BEFORE the column word is read) and i is
// the nearest query of t
__device__ __forceinline__ bool knn_mutual(int t, int i, const uint32_t* __restrict__ colmin, int nt)
{
    if (t < 0 || t >= nt) return false;
    const uint32_t key = colmin[t];
    return key != 0xFFFFFFFFu && (key & 0xFFFFu) == (uint32_t)i;
}
// The one allocator of a MatchWs.  `what`: the member groups the owner needs beyond matching (m_*, mq / mt_idx, xy_*) --
// MATCH_WS_POSE = the 3-D / clique members (pts_*, st_*, clique_ws for kp_cap query keypoints: tens of megabytes at 8000
// features, which is why the monocular alternates go without).  On failure the workspace is given back whole.
enum { MATCH_WS_POSE = 1 };
hipError_t match_ws_alloc(vo_ctx* ctx, vo_ctx::MatchWs& m, int what);
void match_ws_free(vo_ctx::MatchWs& m);
// The one grow step of the workspaces sized on demand (ransac_ws, clique_ws): *ptr holds `need` bytes on return.  A buffer that
// is too small is freed behind a wait for ctx->stream and replaced by max(need, floor) bytes.
int ws_reserve(vo_ctx* ctx, uint8_t** ptr, size_t* bytes, size_t need, size_t floor = 0);
int match_knn2(vo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int32_t* d_idx,
               int32_t* d_dist, int cross = 0, const float* xy_q = nullptr, const float* xy_t = nullptr, float rx = 0.f, float ry = 0.f);
// match_flags of an _ex / fused entry: VO_E_ARG for an unknown bit, and for VO_MATCH_WINDOW while the context has no window
// loop_ok: the entry takes VO_MATCH_LOOP (the stereo pair steps; everywhere else the bit is VO_E_ARG)
int match_flags_check(vo_ctx* ctx, int match_flags, const char* who, bool loop_ok = false);
// The loop check of a stereo pair step (VO_MATCH_LOOP): a match (q, t) is kept only when the right partners of q and t -- the
// slots' kp_rdesc -- are within max_h bits of each other.  Without the flag the pointers are NULL and the kernels run the
// instructions they ran before it existed, behind one uniform branch.
struct LoopGate { const uint8_t *rd_a = nullptr, *rd_b = nullptr; int max_h = 0; };
// -> the gate of a step on slots a and b as the context stands now (the threshold travels by value: a step begun ahead keeps
// it); VO_E_STATE when the flag is set and a slot's keypoints carry no depth
int match_loop_gate(vo_ctx* ctx, const FrameSlot& a, const FrameSlot& b, int match_flags, const char* who, LoopGate* g);
__device__ __forceinline__ bool loop_pass(const uint8_t* __restrict__ rd_q, const uint8_t* __restrict__ rd_t, int q, int t, int loop_max)
{
    const uint4 a0 = ((const uint4*)rd_q)[2 * (size_t)q], a1 = ((const uint4*)rd_q)[2 * (size_t)q + 1];
    const uint4 b0 = ((const uint4*)rd_t)[2 * (size_t)t], b1 = ((const uint4*)rd_t)[2 * (size_t)t + 1];
    const int d = (__popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y)) + (__popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w)) +
                  (__popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y)) + (__popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w));
    return d <= loop_max;
}
// the kNN-2 of a pair step into the current match scratch: slot a's descriptors against slot b's; with VO_MATCH_WINDOW inside
// the context's window around the two slots' keypoint positions
int match_knn2_slots(vo_ctx* ctx, const FrameSlot& a, const FrameSlot& b, int match_flags);
int points3d_launch(vo_ctx* ctx, const int16_t* d_disp16, int w, int h, const float* d_xy, int n,
                    float* d_xyz, uint8_t* d_status);
void host_svd3(const double* A, double* U, double* w, double* Vt);

// ---- stereo PnP pair step (vo_pnp_pair: k_pnp_prep in geom.hip, the rest in ransac.hip) ------------------------------------------
// The record k_pnp_finish writes into pinned host memory; the optional arrays -- mask (1 byte), q, t (int32) for pnp_cap(kp_cap)
// entries each -- lie PNP_HDR bytes behind it in a pose alternate's record, or in the transfer arena for the synchronous call.
struct PnpRec {
    int32_t M, n, best_iter, best_count;   // matches after ratio (+ cross-check), usable correspondences, winner, its inliers
    int32_t flags;                         // bit 0: a 3-D lookup in slot a had no usable tap; bit 1: a match index outside [0, nt)
    int32_t rstatus, rsteps, pad;          // refinement: 0 ok, 1 not requested / not attempted, -1 failed; steps run
    double Rt[12], Rtr[12];                // the winner as vo_ransac_pnp returns it; the refined pose (valid for rstatus 0)
    int32_t lo_rounds, lo_support;         // the LO form only (the plain one leaves them 0): rounds completed, |S_c|
};
static const size_t PNP_HDR = 1024;
static inline size_t pnp_cap(int kp_cap) { return ((size_t)kp_cap + 15) & ~(size_t)15; }
// (PnpDev, the step's device scratch, and PnpWs: ransac_ws.h)
// kNN-2 is done (m_idx / m_dist of the current match scratch): ratio test (+ cross-check), 3-D lookup in slot a, compaction
// nq_dev (may be NULL): a device word that bounds the query rows the kernel looks at (vo_track_map: the rows behind it are padding)
int pnp_prep_launch(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, double ratio, int cross, const PnpDev& d, const LoopGate& g,
                    const int32_t* nq_dev = nullptr);
// The chain as a link of a longer one (vo_track_map).  in: nq_dev as above, rec_dev = device memory that receives a copy of the
// record (the next kernel need not read pinned host memory); out: where the step left its correspondences and their mask
struct PnpChain { const int32_t* nq_dev = nullptr; PnpRec* rec_dev = nullptr; PnpDev d = {}; uint8_t* mask = nullptr; };
// the checks of the PnP pair entries.  view_n >= 0: slot_a is a view slot about to be written with view_n depth-carrying keypoints
// (its present contents are not looked at)
int pnp_check(vo_ctx* ctx, int slot_a, int slot_b, int match_flags, const double* K4v, int iters, float thr, int refine_iters, const char* who,
              LoopGate* lg, int view_n = -1);
// the whole chain on ctx->stream (ransac.hip); rec / arr: pinned host memory k_pnp_finish writes (arr may be NULL)
int pnp_enqueue(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, double ratio, int match_flags, const double* K4v, int iters, float thr, uint32_t seed,
                int refine_iters, PnpRec* rec, uint8_t* arr, const LoopGate& lg, PnpChain* chain = nullptr, int lo_rounds = 0);
// lo_rounds of the _lo entries: 0 .. 8, and a value above 0 needs refine_iters >= 1 (VO_E_ARG otherwise)
int pnp_lo_check(vo_ctx* ctx, int lo_rounds, int refine_iters, const char* who);
// The two halves pnp_enqueue is made of, for a chain with another front (vo_klt_pnp_pair: klt.hip).  pnp_ws_take: the RANSAC
// workspace of the match scratch in force laid out for nq keypoints and iters hypotheses (grown, behind a wait for ctx->stream,
// where it is too small).  pnp_tail_enqueue: everything behind the prep launch -- k_pnp_hyp, k_pnp_score, k_pnp_finish<LO> on
// ctx->stream, reading the compacted (X, uv, hdr, q, t) of w.d; rec / arr / rec_dev as in pnp_enqueue.
int pnp_ws_take(vo_ctx* ctx, int nq, int iters, PnpWs* w);
int pnp_tail_enqueue(vo_ctx* ctx, const PnpWs& w, int nq, const double* K4v, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds,
                     PnpRec* rec, uint8_t* arr, PnpRec* rec_dev);
void pnp_rec_clear(PnpRec* r);
// record (+ arrays) -> the caller's outputs; VO_E_STATE for a pair the step refused.  lo2 (may be NULL) = {rounds completed, |S_c|}
int pnp_unpack(vo_ctx* ctx, const PnpRec* r, const uint8_t* arr, int nq, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
               int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, const char* who, int lo_rounds = 0, int32_t* lo2 = nullptr);
// the ranges pnp_check allows for iters, thr, refine_iters and the focal lengths (VO_E_ARG with its messages)
int pnp_ranges_check(vo_ctx* ctx, const double* K4v, int iters, float thr, int refine_iters, const char* who);
// the link between Lucas-Kanade tracking and the RANSAC (k_klt_pnp_prep, geom.hip): the tracks of slot a's keypoints that ended
// with status 0 (xy_trk / status: KltWs::xy_out / status), their 3-D points in slot a, compacted in keypoint order into d; xy_host
// (may be NULL): pinned host memory that receives the tracked position of each compacted correspondence
int klt_pnp_prep_launch(vo_ctx* ctx, FrameSlot& a, const float* xy_trk, const uint8_t* status, const PnpDev& d, float* xy_host);
// bytes per keypoint of a PnP record's arrays: mask (1), q, t (4 each) and, for a Lucas-Kanade step, the tracked xy (8)
static const size_t PNP_ARR = 17;

// ---- asynchronous steps (match.hip): see vo_ctx::AsyncAlt -------------------------------------------------------------------
static const size_t MONO_HDR = 4096;             // monocular record: [0] M, [1..2] best, E9 at byte 64; arrays from MONO_HDR on
// picks the first free alternate of `kind` from the round-robin position on (-> *k_out), builds every alternate with the first
// step, and orders the alternate's stream behind the main stream and behind whatever still produces the two slots
int alt_open(vo_ctx* ctx, int kind, FrameSlot& a, FrameSlot& b, const char* who, int* k_out);
// The context works on the alternate's stream and in its match scratch for the lifetime of the object, whatever leaves the scope
// (the stream handle changes places with the main one, `mw` is retargeted; no member of a workspace is copied)
struct AltScope {
    vo_ctx* c;
    vo_ctx::AsyncAlt& p;
    AltScope(vo_ctx* c_, vo_ctx::AsyncAlt& p_) : c(c_), p(p_)
    {
        std::swap(c->stream, p.stream);
        c->mw = &p.mw;
    }
    ~AltScope()
    {
        c->mw = &c->main_mw;
        std::swap(c->stream, p.stream);
    }
    AltScope(const AltScope&) = delete;
    AltScope& operator=(const AltScope&) = delete;
};
// the step is enqueued: `done` recorded behind it, both slots get the reader, alternate k is busy and is the ticket
int alt_close(vo_ctx* ctx, int kind, int k, FrameSlot& a, FrameSlot& b, int* ticket_out);
// _end: VO_OK when the caller's own arguments are fine (args_ok) and `ticket` names an open step of `kind` ...
int alt_ticket(vo_ctx* ctx, int kind, int ticket, bool args_ok, const char* who);
// ... which is then closed and waited for
int alt_wait(vo_ctx* ctx, vo_ctx::AsyncAlt& p);
void alt_free(vo_ctx* ctx);                      // every alternate of both kinds and the pose streams
