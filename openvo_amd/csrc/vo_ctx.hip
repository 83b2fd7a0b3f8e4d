// Context, configuration, image front-end (cvtColor / remap), lazy downloads.
// Replaces the cv2 calls of StereoCamera.compute_3d [reference stereo_camera.py:43-55].
#include <stdarg.h>
#include <stdlib.h>
#include "vo_internal.h"

int vo_fail(vo_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

static thread_local std::string g_create_err;
static int lanes_ensure(vo_ctx* ctx);

// ---- pinned transfer arena ---------------------------------------------------------------
static const size_t ARENA_BASE = 4096;

static void* arena_take(vo_ctx* ctx, size_t bytes)
{
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (ARENA_BASE + ctx->arena_off + need > ctx->pinned_bytes) return nullptr;
    void* p = (char*)ctx->pinned + ARENA_BASE + ctx->arena_off;
    ctx->arena_off += need;
    return p;
}

void* xfer_stage(vo_ctx* ctx, size_t bytes) { return arena_take(ctx, bytes); }

int xfer_flush(vo_ctx* ctx)
{
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (const auto& c : ctx->pending) memcpy(c.dst, c.src, c.bytes);
    ctx->pending.clear();
    ctx->arena_off = 0;
    return VO_OK;
}

int xfer_h2d(vo_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes)
{
    if (bytes == 0) return VO_OK;
    void* st = arena_take(ctx, bytes);
    if (!st && bytes + 64 <= ctx->pinned_bytes - ARENA_BASE) {
        int rc = xfer_flush(ctx);  // arena full: drain what is in flight, then reuse it
        if (rc) return rc;
        st = arena_take(ctx, bytes);
    }
    if (!st) {  // larger than the arena: plain copy
        VO_HIP(ctx, hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return VO_OK;
    }
    memcpy(st, host_src, bytes);
    VO_HIP(ctx, hipMemcpyAsync(dev_dst, st, bytes, hipMemcpyHostToDevice, ctx->stream));
    return VO_OK;
}

int xfer_d2h(vo_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes)
{
    if (bytes == 0) return VO_OK;
    void* st = arena_take(ctx, bytes);
    if (!st && bytes + 64 <= ctx->pinned_bytes - ARENA_BASE) {
        int rc = xfer_flush(ctx);
        if (rc) return rc;
        st = arena_take(ctx, bytes);
    }
    if (!st) {
        VO_HIP(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return VO_OK;
    }
    VO_HIP(ctx, hipMemcpyAsync(st, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->pending.push_back({host_dst, st, bytes});
    return VO_OK;
}

template <typename T>
static int dalloc(vo_ctx* ctx, T** p, size_t count)
{
    VO_HIP(ctx, hipMalloc((void**)p, count * sizeof(T) + 256));
    return VO_OK;
}
#define DALLOC(p, n)                         \
    do {                                     \
        int rc__ = dalloc(ctx, &(p), (n));   \
        if (rc__) { g_create_err = ctx->err; vo_destroy(ctx); return rc__; } \
    } while (0)

extern "C" const char* vo_last_error(const vo_ctx* ctx)
{
    return ctx ? ctx->err.c_str() : g_create_err.c_str();
}

int orb_ws_alloc(vo_ctx* ctx, OrbWs& o)
{
    const size_t cand = (size_t)ctx->cand_cap * 4 * sizeof(int32_t);   // 8 levels together: < 3.2x level 0
    void** ps[] = { (void**)&o.pyr_img, (void**)&o.pyr_mask,
                    (void**)&o.cand_pos, (void**)&o.cand_resp, (void**)&o.candA_pos, (void**)&o.candA_resp, (void**)&o.candB_pos,
                    (void**)&o.candB_resp, (void**)&o.counters };
    const size_t sz[] = { ctx->pyr_bytes, ctx->pyr_bytes, cand, cand, cand, cand, cand,
                          cand, 8192 * 4 };
    for (size_t k = 0; k < sizeof(ps) / sizeof(ps[0]); k++)
        if (hipMalloc(ps[k], sz[k] + 256) != hipSuccess) return VO_E_HIP;
    return VO_OK;
}

void orb_ws_free(OrbWs& o)
{
    void* ps[] = { o.pyr_img, o.pyr_mask, o.cand_pos, o.cand_resp, o.candA_pos, o.candA_resp,
                   o.candB_pos, o.candB_resp, o.counters };
    for (void* p : ps) if (p) (void)hipFree(p);
    o = OrbWs();
}

// The one allocator of an SGBM workspace (the main one in vo_create, an engine's on that engine's first use): what a disparity
// run writes, and the `done` event.  sw_bnd comes with the first diagonal sweep (sgbm.hip).  A partly built workspace is given
// back whole.  The ORB scratch, staging and events of the ENGINE that sit in the same struct are engine_prepare's.
static void sgbm_ws_free(vo_ctx::SgbmWs& a)
{
    void** ps[] = { (void**)&a.planesL, (void**)&a.planesR, (void**)&a.C, (void**)&a.S, (void**)&a.sw_ctl, (void**)&a.disp_tmp,
                    (void**)&a.ccl_runlen, (void**)&a.ccl_label, (void**)&a.ccl_size, (void**)&a.rec, (void**)&a.sw_bnd };
    for (void** q : ps) { if (*q) (void)hipFree(*q); *q = nullptr; }
    if (a.done) (void)hipEventDestroy(a.done);
    a.done = nullptr;
    a.S_vols = 0; a.sw_bnd_bytes = 0; a.ready = false; a.done_valid = false;
}

static hipError_t sgbm_ws_alloc(vo_ctx* ctx, vo_ctx::SgbmWs& a)
{
    const size_t npx = (size_t)ctx->max_w * ctx->max_h;
    const int vols = 3;                          // L_W + L_E, MODE_HH's reverse-pass sum, checkpoints (ensure_S grows it for uniquenessRatio >= 100)
    void** ps[] = { (void**)&a.planesL, (void**)&a.planesR, (void**)&a.C, (void**)&a.S, (void**)&a.sw_ctl, (void**)&a.disp_tmp,
                    (void**)&a.ccl_runlen, (void**)&a.ccl_label, (void**)&a.ccl_size, (void**)&a.rec };
    const size_t sz[] = { npx * 2 * 4, npx * 6 * 4, ctx->vol_cells * 2, ctx->vol_cells * 2 * vols, ctx->sw_ctl_words * sizeof(int), npx * 2,
                          npx * 4, npx * 4, npx * 4, (npx + 64) * 8 };
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < sizeof(ps) / sizeof(ps[0]) && e == hipSuccess; k++) e = hipMalloc(ps[k], sz[k] + 256);
    if (e == hipSuccess) e = dev_zero(a.sw_ctl, ctx->sw_ctl_words * sizeof(int));      // (the first sweep runs on an engine's or the main stream)
    if (e == hipSuccess && !a.done) e = hipEventCreateWithFlags(&a.done, hipEventDisableTiming);
    if (e != hipSuccess) { sgbm_ws_free(a); return e; }
    a.S_vols = vols;
    a.ready = true;
    return hipSuccess;
}

int lds_allow_big(vo_ctx* ctx, const void* fn)
{
    for (const void* f : ctx->big_lds) if (f == fn) return VO_OK;
    VO_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ctx->big_lds.push_back(fn);
    return VO_OK;
}

extern "C" int vo_create(int device_id, int max_w, int max_h, int max_disp, int max_kp, vo_ctx** out)
{
    if (!out) return VO_E_ARG;
    *out = nullptr;
    if (max_w < 64 || max_h < 64 || max_disp < 16 || max_disp > 256 || max_disp % 16 || max_kp < 16) {
        g_create_err = "vo_create: need max_w,max_h >= 64, 16 <= max_disp <= 256 (multiple of 16), max_kp >= 16";
        return VO_E_ARG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("vo_create: no HIP device available (") + hipGetErrorString(e) +
                       "); libvo355 has no CPU fallback";
        return VO_E_HIP;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_err = "vo_create: bad device id"; return VO_E_ARG; }
    vo_ctx* ctx = new vo_ctx();
    ctx->device = device_id;
    ctx->max_w = max_w; ctx->max_h = max_h; ctx->max_disp = max_disp; ctx->max_kp = max_kp;
    if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_err = hipGetErrorString(e); delete ctx; return VO_E_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        // (some driver stacks report no marketing name: say what the device is by its architecture and size then)
        char generic[96];
        snprintf(generic, sizeof(generic), "AMD GPU, %d CUs, %.0f GB", prop.multiProcessorCount, (double)prop.totalGlobalMem / 1e9);
        snprintf(ctx->devname, sizeof(ctx->devname), "%s (%s)", prop.name[0] ? prop.name : generic, prop.gcnArchName);
    }
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) { g_create_err = hipGetErrorString(e); delete ctx; return VO_E_HIP; }
    // The hardware queues this process may open decide whether the look-ahead pairs' sweeps are grouped (sweep_group_size), and
    // where they are -- by the budget or by VO_SWEEP_GROUP -- the two lane streams come right here: the runtime maps streams onto
    // hardware queues in the order they are created and first used, so with four queues the main stream and the two lanes lie
    // on three different ones and the null stream (dev_zero below) with the pose streams on the fourth (measured: created at
    // the end of this function, a lane shared its queue with the pose stream and the flagship lost 9 % instead of gaining 7 %).
    // A context with a queue per stream creates none, now or later, unless a setter puts groups in force.
    // VO_GROUP_LANES=0: no lanes, sweep groups keep to the engines' own streams.
    if (const char* e8 = getenv("VO_ENGINES")) { int v = atoi(e8); if (v >= 1 && v <= vo_ctx::MAX_ENGINES) ctx->n_engines = v; }
    if (const char* eq = getenv("GPU_MAX_HW_QUEUES")) { int v = atoi(eq); if (v >= 1) ctx->hw_queues = v; }
    if (const char* eg = getenv("VO_SWEEP_GROUP")) { int v = atoi(eg); if (v >= 1 && v <= VO_MAX_SWEEP_GROUP) ctx->sweep_group_req = v; }
    if (const char* el = getenv("VO_GROUP_LANES")) ctx->lanes_on = atoi(el) != 0;
    if (const char* ef = getenv("VO_GROUP_FRONTS")) { int v = atoi(ef); if (v >= 0) ctx->front_batch = v > VO_MAX_SWEEP_GROUP ? VO_MAX_SWEEP_GROUP : v; }
    if (lanes_ensure(ctx)) { g_create_err = "hipStreamCreate failed (lane streams)"; vo_destroy(ctx); return VO_E_HIP; }
    (void)hipEventCreate(&ctx->ev0);
    (void)hipEventCreate(&ctx->ev1);

    const size_t npx = (size_t)max_w * max_h;
    // keypoint capacity: OpenCV keeps response ties, so allow head-room over nfeatures
    ctx->kp_cap = max_kp * 2 + 1024;
    for (int s = 0; s <= VO_NUM_SLOTS; s++) {
        FrameSlot& f = ctx->slots[s];
        DALLOC(f.left, npx); DALLOC(f.right, npx); DALLOC(f.disp16, npx);
        (void)hipEventCreateWithFlags(&f.ready, hipEventDisableTiming);
        DALLOC(f.kp_xy, (size_t)ctx->kp_cap * 2); DALLOC(f.kp_size, ctx->kp_cap); DALLOC(f.kp_angle, ctx->kp_cap);
        DALLOC(f.kp_resp, ctx->kp_cap); DALLOC(f.kp_oct, ctx->kp_cap); DALLOC(f.desc, (size_t)ctx->kp_cap * 32);
        DALLOC(f.mono_depth, ctx->kp_cap); DALLOC(f.mono_serial_dev, 16);
        DALLOC(f.kp_xyz, (size_t)ctx->kp_cap * 3); DALLOC(f.kp_disp, ctx->kp_cap); DALLOC(f.kp_rdesc, (size_t)ctx->kp_cap * 32);
        if (dev_zero(f.mono_serial_dev, 64) != hipSuccess) { g_create_err = "clearing a slot's depth serial failed"; vo_destroy(ctx); return VO_E_HIP; }
    }
    {
        FrameSlot& r = ctx->sparse_r;      // the second scratch keypoint set of vo_sparse_stereo
        DALLOC(r.kp_xy, (size_t)ctx->kp_cap * 2); DALLOC(r.kp_size, ctx->kp_cap); DALLOC(r.kp_angle, ctx->kp_cap);
        DALLOC(r.kp_resp, ctx->kp_cap); DALLOC(r.kp_oct, ctx->kp_cap); DALLOC(r.desc, (size_t)ctx->kp_cap * 32);
        ctx->sp_main.l = &ctx->slots[VO_NUM_SLOTS]; ctx->sp_main.r = &r;      // (the rest of it comes with the first sparse call: sparse_ws_prepare)
    }
    ctx->stage_bytes = npx * 3;
    DALLOC(ctx->stage_in, ctx->stage_bytes * 2);
    for (int c = 0; c < 2; c++) { DALLOC(ctx->map1[c], npx * 2); DALLOC(ctx->map2[c], npx); }
    ctx->vol_cells = npx * (size_t)((max_disp + 31) & ~31);
    ctx->sw_ctl_words = 2 * 2048;                        // two control blocks: {work items taken, sticky error, ...} + per-strip timeline
    if (sgbm_ws_alloc(ctx, ctx->main_ws) != hipSuccess) { g_create_err = "hipMalloc failed (SGBM workspace)"; vo_destroy(ctx); return VO_E_HIP; }
    DALLOC(ctx->dump, 4096);
    // ORB: 8-level pyramid is < 3.2x the base image
    ctx->pyr_bytes = npx * 4;
    DALLOC(ctx->rs_ofs, (size_t)(max_w + max_h) * 2 * VO_ORB_LEVELS);
    DALLOC(ctx->rs_coef, (size_t)(max_w + max_h) * 4 * VO_ORB_LEVELS);
    DALLOC(ctx->pyr_rects, 4096);
    // FAST candidates after NMS are never 8-adjacent: at most ceil(w/2)*ceil(h/2) per level
    ctx->cand_cap = (int)((size_t)((max_w + 1) / 2) * ((max_h + 1) / 2));
    // (summed over the 8 levels: < 3.2x that)
    if (orb_ws_alloc(ctx, (*ctx->orbws))) { g_create_err = "hipMalloc failed (ORB workspace)"; vo_destroy(ctx); return VO_E_HIP; }
    DALLOC(ctx->host_mask_dev, npx);
    DALLOC(ctx->mq, (size_t)ctx->kp_cap * 32); DALLOC(ctx->mt, (size_t)ctx->kp_cap * 32);
    if (match_ws_alloc(ctx, ctx->main_mw, MATCH_WS_POSE) != hipSuccess) { g_create_err = "hipMalloc failed (match scratch)"; vo_destroy(ctx); return VO_E_HIP; }
    DALLOC(ctx->red, 4096);
    ctx->pinned_bytes = 8 << 20;
    if (hipHostMalloc(&ctx->pinned, ctx->pinned_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&ctx->slot_words, 256 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
        g_create_err = "hipHostMalloc failed"; vo_destroy(ctx); return VO_E_HIP;
    }
    memset(ctx->slot_words, 0, 256 * sizeof(int32_t));
    // one count word per slot, then one sweep word per slot from word 64 on, then four words of sparse record per slot from word 128 on
    static_assert(128 + 4 * (VO_NUM_SLOTS + 1) <= 256 && VO_NUM_SLOTS + 1 <= 32, "slot_words layout");
    for (int s = 0; s <= VO_NUM_SLOTS; s++) {
        ctx->slots[s].n_kp_host = ctx->slot_words + s; ctx->slots[s].sweep_word = ctx->slot_words + 64 + s;
        ctx->slots[s].sp_rec = ctx->slot_words + 128 + 4 * s;
    }
    ctx->sparse_r.n_kp_host = ctx->slot_words + 32;      // (words 29 .. 63 belong to no slot)
    DALLOC(ctx->d_sweep_errs, 64);
    if (dev_zero(ctx->d_sweep_errs, 64 * sizeof(int)) != hipSuccess) { g_create_err = "clearing the sweep error counter failed"; vo_destroy(ctx); return VO_E_HIP; }
    {
        // every engine owns a full SGBM workspace: cost volume + 3 aggregated volumes + boundary granules (< 1 volume) + planes.
        // Keep all of them within 40 % of what the device has free right now (frame slots, ORB scratch and the caller's staged
        // inputs need room too).
        const double per_engine = (double)ctx->vol_cells * 2.0 * 5.0 + (double)npx * 64.0;
        size_t free_b = 0, total_b = 0;
        double budget = 96e9;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = 0.4 * (double)free_b;
        const int fit = (int)(budget / per_engine);
        ctx->engines_fit = fit < 2 ? 2 : fit;
        if (ctx->n_engines > ctx->engines_fit) ctx->n_engines = ctx->engines_fit;
    }
    if (const char* e9 = getenv("VO_POSE_STREAMS")) { int v = atoi(e9); if (v >= 1 && v <= vo_ctx::N_POSE_STREAMS) { ctx->n_pose_streams = v; ctx->pose_streams_env = true; } }
    if (const char* e27 = getenv("VO_STAGGER")) ctx->tune_stagger = atoi(e27);
    if (const char* e25 = getenv("VO_DIAG_WAVES")) { const int v = atoi(e25); ctx->tune_diag_nwc = (v == 7 || v == 11 || v == 15) ? v : 0; }   // the three strip widths that are built
#ifdef VO_TEST_HOOKS
    // development switches live in the test-only build alone (libvo355_hooks.so; tools/stage_ablation.py loads it): some of them
    // switch stages or the strip hand-off OFF, and nothing in a user's environment may make the product compute garbage
    if (const char* e27 = getenv("VO_DIAG_WGS")) ctx->tune_diag_wgs = atoi(e27);
    if (const char* e26 = getenv("VO_DIAG_DEBUG")) ctx->tune_diag_dbg = atoi(e26);
    if (const char* e10 = getenv("VO_FAULT_PREFETCH")) ctx->fault_prefetch = atoi(e10);   // test-only build (libvo355_hooks.so)
    if (const char* e11 = getenv("VO_FAULT_SWEEP")) ctx->fault_sweep = atoi(e11);
    if (const char* e12 = getenv("VO_FAULT_PNP_RANGE")) ctx->fault_pnp_range = atoi(e12);
    if (const char* e13 = getenv("VO_FAULT_MAP_NAN")) ctx->fault_map_nan = atoi(e13);
#endif
    if (const char* e6 = getenv("VO_SWEEP_TY")) { int v = atoi(e6); if (v >= 4 && v <= 4096) ctx->tune_sweep_ty = v; }
    // (the memory bound above may have put groups in force that the request alone did not)
    if (lanes_ensure(ctx)) { g_create_err = "hipStreamCreate failed (lane streams)"; vo_destroy(ctx); return VO_E_HIP; }
    *out = ctx;
    return VO_OK;
}

// the two lane streams exist once the group size in force is above 1 (lane_mode)
static int lanes_ensure(vo_ctx* ctx)
{
    if (!ctx->lanes_on || sweep_group_size(ctx) <= 1) return VO_OK;
    for (hipStream_t& l : ctx->lane)
        if (!l) VO_HIP(ctx, hipStreamCreateWithFlags(&l, hipStreamNonBlocking));
    // ... and the first pose stream behind them -- the one the pose steps keep to beside the lanes (pose_stream_count) -- so
    // that it takes the queue after the lanes' whatever the number of engine streams created before the first pose step
    if (!ctx->pose_streams[0]) VO_HIP(ctx, hipStreamCreateWithFlags(&ctx->pose_streams[0], hipStreamNonBlocking));
    return VO_OK;
}

extern "C" void vo_destroy(vo_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)sweep_group_close(ctx, VO_GRP_OTHER);      // (its members' slots are mid-run: finished like any other work in flight)
    sweep_group_free(ctx);
    if (ctx->stage_thread.joinable()) {
        { std::lock_guard<std::mutex> lk(ctx->stage_mu); ctx->stage_stop = true; }
        ctx->stage_cv.notify_all();
        ctx->stage_thread.join();
    }
    (void)engine_streams_sync(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int s = 0; s <= VO_NUM_SLOTS; s++) {
        FrameSlot& f = ctx->slots[s];
        void* ps[] = { f.left, f.right, f.disp16, f.kp_xy, f.kp_size, f.kp_angle, f.kp_resp, f.kp_oct, f.desc, f.mono_depth, f.mono_serial_dev,
                       f.kp_xyz, f.kp_disp, f.kp_rdesc };
        for (void* p : ps) if (p) (void)hipFree(p);
        if (f.ready) (void)hipEventDestroy(f.ready);
    }
    void* ps[] = { ctx->stage_in, ctx->map1[0], ctx->map1[1], ctx->map2[0], ctx->map2[1], ctx->dump, ctx->rs_ofs, ctx->rs_coef, ctx->pyr_rects,
                   ctx->host_mask_dev, ctx->mq, ctx->mt, ctx->red, ctx->img3_ws, ctx->d_sweep_errs, ctx->sparse_r.kp_xy, ctx->sparse_r.kp_size,
                   ctx->sparse_r.kp_angle, ctx->sparse_r.kp_resp, ctx->sparse_r.kp_oct, ctx->sparse_r.desc };
    for (void* p : ps) if (p) (void)hipFree(p);
    alt_free(ctx);
    for (LandmarkMap& m : ctx->maps) map_free(m);
    sparse_ws_free(ctx->sp_main);
    for (SparseWs& w : ctx->sp_alt) sparse_ws_free(w);
    match_ws_free(ctx->main_mw);
    sgbm_ws_free(ctx->main_ws);
    orb_ws_free(ctx->main_ws.orb);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->slot_words) (void)hipHostFree(ctx->slot_words);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->staged) (void)hipFree(ctx->staged);
    for (int k = 0; k < vo_ctx::MAX_ENGINES; k++) {
        vo_ctx::SgbmWs& a = ctx->ws_alt[k];
        sgbm_ws_free(a);
        orb_ws_free(a.orb);
        if (ctx->la_stage[k]) (void)hipFree(ctx->la_stage[k]);
        if (a.pinned) (void)hipHostFree(a.pinned);
        if (a.h2d_done) (void)hipEventDestroy(a.h2d_done);
        if (a.mid) (void)hipEventDestroy(a.mid);
        if (a.swept) (void)hipEventDestroy(a.swept);
        if (a.moved) (void)hipEventDestroy(a.moved);
        if (ctx->la_stream[k]) (void)hipStreamDestroy(ctx->la_stream[k]);
    }
    for (vo_ctx::HostStage& hs : ctx->host_stage) {
        if (hs.pinned) (void)hipHostFree(hs.pinned);
        if (hs.h2d_done) (void)hipEventDestroy(hs.h2d_done);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (hipStream_t l : ctx->lane) if (l) (void)hipStreamDestroy(l);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int vo_set_engines(vo_ctx* ctx, int n)
{
    if (!ctx) return VO_E_ARG;
    if (n > 0) {
        if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;
        if (n > vo_ctx::MAX_ENGINES) n = vo_ctx::MAX_ENGINES;
        if (n > ctx->engines_fit) n = ctx->engines_fit;
        ctx->n_engines = n;
        ctx->next_engine %= n;          // (the stagger wait and the monocular span index modulo n_engines: nothing else remembers one)
        if (int rc = lanes_ensure(ctx)) return rc;
    }
    return ctx->n_engines;
}

// How many look-ahead pairs share one diagonal sweep launch (see vo_ctx::grp).  n <= 0 only asks; otherwise n (clamped to
// VO_MAX_SWEEP_GROUP) is the request from now on and the open group is closed.  Returns the size in force.
extern "C" int vo_set_sweep_group(vo_ctx* ctx, int n)
{
    if (!ctx) return VO_E_ARG;
    if (n > 0) {
        if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;
        ctx->sweep_group_req = n > VO_MAX_SWEEP_GROUP ? VO_MAX_SWEEP_GROUP : n;
        if (int rc = lanes_ensure(ctx)) return rc;
    }
    return sweep_group_size(ctx);
}

// no further look-ahead pair follows now: the open group, if any, is swept as it stands
extern "C" int vo_lookahead_flush(vo_ctx* ctx)
{
    if (!ctx) return VO_E_ARG;
    if (sweep_group_members(ctx) > 0) {
        VO_HIP(ctx, hipSetDevice(ctx->device));
        if (int rc = sweep_group_close(ctx, VO_GRP_FLUSH)) return rc;
    }
    return sweep_group_size(ctx);
}

extern "C" int vo_sweep_group_stats(vo_ctx* ctx, int64_t* closed4, int* open_members)
{
    if (!ctx || !closed4) return vo_fail(ctx, VO_E_ARG, "vo_sweep_group_stats: bad argument");
    for (int i = 0; i < 4; i++) closed4[i] = ctx->grp_closed[i];
    if (open_members) *open_members = sweep_group_members(ctx);
    return VO_OK;
}

extern "C" int vo_device_name(const vo_ctx* ctx, char* buf, int buflen)
{
    if (!ctx || !buf || buflen <= 0) return VO_E_ARG;
    snprintf(buf, buflen, "%s", ctx->devname);
    return VO_OK;
}

extern "C" int vo_synchronize(vo_ctx* ctx)
{
    if (!ctx) return VO_E_ARG;
    if (int rc = sweep_group_close(ctx, VO_GRP_CONSUMER)) return rc;
    VO_HIP(ctx, engine_streams_sync(ctx));
    for (int kind : { vo_ctx::ALT_POSE, vo_ctx::ALT_MONO })
        for (int k = 0; k < vo_ctx::alt_count(kind); k++)
            if (ctx->alt(kind, k).stream) VO_HIP(ctx, hipStreamSynchronize(ctx->alt(kind, k).stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_set_rectify_maps(vo_ctx* ctx, int cam, const int16_t* map1, const uint16_t* map2, int w, int h)
{
    if (!ctx || cam < 0 || cam > 1 || !map1 || !map2) return vo_fail(ctx, VO_E_ARG, "vo_set_rectify_maps: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w <= 0 || h <= 0) return vo_fail(ctx, VO_E_CAP, "maps %dx%d exceed context %dx%d", w, h, ctx->max_w, ctx->max_h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    VO_HIP(ctx, hipMemcpyAsync(ctx->map1[cam], map1, (size_t)w * h * 4, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(ctx->map2[cam], map2, (size_t)w * h * 2, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->map_w = w; ctx->map_h = h; ctx->has_map[cam] = true;
    return VO_OK;
}

extern "C" int vo_set_sgbm(vo_ctx* ctx, int minDisparity, int numDisparities, int blockSize, int P1, int P2,
                           int disp12MaxDiff, int preFilterCap, int uniquenessRatio, int speckleWindowSize,
                           int speckleRange, int mode)
{
    if (!ctx) return VO_E_ARG;
    if (numDisparities <= 0 || numDisparities % 16) return vo_fail(ctx, VO_E_ARG, "numDisparities must be a positive multiple of 16");
    if (numDisparities > ctx->max_disp) return vo_fail(ctx, VO_E_CAP, "numDisparities %d > max_disp %d", numDisparities, ctx->max_disp);
    if (mode != 0 && mode != 1 && mode != 2) return vo_fail(ctx, VO_E_ARG, "mode must be 0 (MODE_SGBM), 1 (MODE_HH) or 2 (MODE_SGBM_3WAY)");
    if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;     // its members finish under the parameters they began with
    // effective parameters exactly as computeDisparitySGBM derives them
    SgbmEff& e = ctx->sg;
    e.minD = minDisparity; e.D = numDisparities; e.maxD = minDisparity + numDisparities;
    e.ur = uniquenessRatio >= 0 ? uniquenessRatio : 10;
    e.d12 = disp12MaxDiff > 0 ? disp12MaxDiff : 1;
    e.P1 = P1 > 0 ? P1 : 2;
    int p2 = P2 > 0 ? P2 : 5;
    e.P2 = p2 > e.P1 + 1 ? p2 : e.P1 + 1;
    int bs = blockSize > 0 ? blockSize : 5;
    e.SW2 = e.SH2 = bs / 2;
    e.ftzero = (preFilterCap > 15 ? preFilterCap : 15) | 1;
    e.speckleWindow = speckleWindowSize; e.speckleRange = speckleRange; e.mode = mode;
    if (e.SW2 > 5) return vo_fail(ctx, VO_E_ARG, "blockSize > 11 is not supported");
    if (e.P2 > 8000 || e.ftzero > 127) return vo_fail(ctx, VO_E_ARG, "P2 > 8000 or preFilterCap > 127 would overflow int16 costs");
    // a path cost is at most the block's largest matching cost + P2; OpenCV keeps it in a short and wraps beyond 32767 (its
    // results are then garbage): refused here rather than reproduced
    {
        const int side = 2 * e.SW2 + 1, cmax = side * side * (2 * e.ftzero + 63);
        if (cmax + e.P2 > 32767)
            return vo_fail(ctx, VO_E_ARG, "blockSize %d with preFilterCap %d and P2 %d lets a path cost reach %d: beyond the int16 OpenCV computes in",
                           side, e.ftzero, e.P2, cmax + e.P2);
    }
    e.set = true;
    return VO_OK;
}

// The matching cost of the SGBM front (include/vo355.h).  Lives beside SgbmEff and outlives vo_set_sgbm.
extern "C" int vo_set_sgbm_cost(vo_ctx* ctx, int cost, int census_w, int census_h)
{
    if (!ctx) return VO_E_ARG;
    if (cost != VO_SGBM_COST_BT && cost != VO_SGBM_COST_CENSUS) return vo_fail(ctx, VO_E_ARG, "cost must be 0 (VO_SGBM_COST_BT) or 1 (VO_SGBM_COST_CENSUS)");
    if (cost == VO_SGBM_COST_CENSUS) {
        const bool w_ok = census_w == 3 || census_w == 5 || census_w == 7 || census_w == 9;
        const bool h_ok = census_h == 3 || census_h == 5 || census_h == 7;
        if (!w_ok || !h_ok) return vo_fail(ctx, VO_E_ARG, "census window %d x %d: the width must be 3, 5, 7 or 9 and the height 3, 5 or 7", census_w, census_h);
    } else {
        census_w = ctx->sg_cost.cw; census_h = ctx->sg_cost.ch;      // (ignored with BT: the window on record stays)
    }
    if (cost == ctx->sg_cost.cost && census_w == ctx->sg_cost.cw && census_h == ctx->sg_cost.ch) return VO_OK;
    if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;     // its members finish under the cost they began with
    ctx->sg_cost.cost = cost; ctx->sg_cost.cw = census_w; ctx->sg_cost.ch = census_h;
    return VO_OK;
}

extern "C" int vo_get_sgbm_cost(const vo_ctx* ctx, int* cost, int* census_w, int* census_h)
{
    if (!ctx || !cost || !census_w || !census_h) return VO_E_ARG;
    *cost = ctx->sg_cost.cost;
    *census_w = ctx->sg_cost.cw;
    *census_h = ctx->sg_cost.ch;
    return VO_OK;
}

// C of the latest synchronous run in the main workspace as [H][W1][D]: the padding to Dp stays behind
extern "C" int vo_sgbm_cost_volume(vo_ctx* ctx, int16_t* out, size_t cells)
{
    if (!ctx || !out) return vo_fail(ctx, VO_E_ARG, "vo_sgbm_cost_volume: bad argument");
    if (!ctx->c_last.valid || !ctx->main_ws.C) return vo_fail(ctx, VO_E_STATE, "vo_sgbm_cost_volume: no synchronous run has left a cost volume in the main workspace");
    const size_t rows = (size_t)ctx->c_last.H * ctx->c_last.W1;
    if (cells != rows * ctx->c_last.D) return vo_fail(ctx, VO_E_ARG, "vo_sgbm_cost_volume: %zu cells asked for, the volume has %zu", cells, rows * ctx->c_last.D);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VO_HIP(ctx, hipMemcpy2D(out, (size_t)ctx->c_last.D * 2, ctx->main_ws.C, (size_t)ctx->c_last.Dp * 2, (size_t)ctx->c_last.D * 2, rows, hipMemcpyDeviceToHost));
    return VO_OK;
}

// Q or the ROI changes: a sparse chain begun ahead ran with the old one.  Its result is no longer what vo_sparse_stereo would
// compute: the next call on such a slot recomputes (the chain itself finishes; the slot's `ready` still orders its consumers).
static void sparse_void_ahead(vo_ctx* ctx)
{
    for (int s = 0; s < VO_NUM_SLOTS; s++) { ctx->slots[s].sp_pending = false; ctx->slots[s].sp_ahead = false; }
}

extern "C" int vo_set_Q(vo_ctx* ctx, const double* Q16)
{
    if (!ctx || !Q16) return VO_E_ARG;
    memcpy(ctx->Q, Q16, sizeof(ctx->Q));
    ctx->has_Q = true;
    sparse_void_ahead(ctx);
    return VO_OK;
}

extern "C" int vo_set_roi(vo_ctx* ctx, int x0, int y0, int x1, int y1)
{
    if (!ctx) return VO_E_ARG;
    if (x0 < 0 || y0 < 0) return vo_fail(ctx, VO_E_ARG, "negative ROI origin is not supported");
    if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;
    ctx->roi[0] = x0; ctx->roi[1] = y0; ctx->roi[2] = x1; ctx->roi[3] = y1;
    ctx->has_roi = true;
    sparse_void_ahead(ctx);
    return VO_OK;
}

// ---- cvtColor BGR2GRAY (OpenCV 4.x RGB2Gray<uchar>, 15-bit coefficients) -------------
__global__ void k_bgr2gray(const uint8_t* __restrict__ bgr, int n, uint8_t* __restrict__ gray)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int b = bgr[3 * (size_t)i], g = bgr[3 * (size_t)i + 1], r = bgr[3 * (size_t)i + 2];
    gray[i] = (uint8_t)((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15);
}

// ---- remap INTER_LINEAR with CV_16SC2 + fractional maps, border constant 0 ------------
__global__ void k_remap(const uint8_t* __restrict__ src, int sw, int sh, const int16_t* __restrict__ map1,
                        const uint16_t* __restrict__ map2, int w, int h, uint8_t* __restrict__ dst)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    size_t i = (size_t)y * w + x;
    int sx = map1[2 * i], sy = map1[2 * i + 1];
    int f = map2[i] & 1023, fx = f & 31, fy = f >> 5;
    int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    int p00 = 0, p01 = 0, p10 = 0, p11 = 0;
    bool x0ok = (unsigned)sx < (unsigned)sw, x1ok = (unsigned)(sx + 1) < (unsigned)sw;
    if ((unsigned)sy < (unsigned)sh) {
        if (x0ok) p00 = src[(size_t)sy * sw + sx];
        if (x1ok) p01 = src[(size_t)sy * sw + sx + 1];
    }
    if ((unsigned)(sy + 1) < (unsigned)sh) {
        if (x0ok) p10 = src[(size_t)(sy + 1) * sw + sx];
        if (x1ok) p11 = src[(size_t)(sy + 1) * sw + sx + 1];
    }
    int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
    dst[i] = (uint8_t)min(v, 255);
}

static int check_slot(vo_ctx* ctx, int slot)
{
    if (!ctx) return VO_E_ARG;
    if (slot < 0 || slot >= VO_NUM_SLOTS) return vo_fail(ctx, VO_E_ARG, "slot %d out of range [0,%d)", slot, VO_NUM_SLOTS);
    return VO_OK;
}

// upload one camera image into dst (gray, rectified)
// Image bytes out of pinned host memory by a kernel (the GPU reads them over the host link itself).  An asynchronous
// hipMemcpy from pinned memory goes to a DMA engine instead, and every hand-over between that engine's queue and the compute
// queue of the look-ahead engine costs the stream tens of microseconds -- with a dozen engines uploading, the from-host rate
// fell to 0.6-0.8 of the resident rate.
typedef uint32_t ingest_u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_ingest_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t bytes)
{
    const size_t n16 = bytes / 16, stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < n16; i += stride)
        ((ingest_u32x4*)dst)[i] = __builtin_nontemporal_load((const ingest_u32x4*)src + i);
    for (size_t i = n16 * 16 + i0; i < bytes; i += stride) dst[i] = src[i];
}

static int ingest_bytes(vo_ctx* ctx, uint8_t* dst, const uint8_t* src, size_t bytes, hipMemcpyKind kind, bool by_kernel)
{
    if (by_kernel && ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0)) {
        const int blocks = (int)((bytes / 16 + 255) / 256 < 2048 ? (bytes / 16 + 255) / 256 : 2048);
        hipLaunchKernelGGL(k_ingest_copy, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, ctx->stream, src, dst, bytes);
        return VO_OK;
    }
    VO_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    return VO_OK;
}

static int ingest(vo_ctx* ctx, int cam, const uint8_t* host, int w, int h, int channels, int preprocessed, uint8_t* dst,
                  uint8_t* stage, hipMemcpyKind kind = hipMemcpyHostToDevice, bool by_kernel = false)
{
    const size_t n = (size_t)w * h;
    const bool need_remap = !preprocessed;
    if (need_remap && (!ctx->has_map[cam] || ctx->map_w != w || ctx->map_h != h))
        return vo_fail(ctx, VO_E_STATE, "rectification maps for camera %d not set for %dx%d", cam, w, h);
    uint8_t* gray = need_remap ? stage + n * 3 : dst;  // gray staging behind the colour staging
    if (channels == 3) {
        if (int rcb = ingest_bytes(ctx, stage, host, n * 3, kind, by_kernel)) return rcb;
        hipLaunchKernelGGL(k_bgr2gray, dim3(div_up((int)n, 256)), dim3(256), 0, ctx->stream, stage, (int)n, gray);
    } else {
        if (int rcb = ingest_bytes(ctx, gray, host, n, kind, by_kernel)) return rcb;
    }
    if (need_remap)
        hipLaunchKernelGGL(k_remap, dim3(div_up(w, 256), h), dim3(256), 0, ctx->stream, gray, w, h, ctx->map1[cam],
                           ctx->map2[cam], w, h, dst);
    VO_CHECK_LAUNCH(ctx);
    return VO_OK;
}

extern "C" int vo_upload_pair(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h,
                              int channels, int preprocessed)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!left || !right || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_upload_pair: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& f = ctx->slots[slot];
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;
    StageTimer t(ctx, VO_T_UPLOAD);
    // the two cameras use disjoint halves of the staging buffer (4 bytes/pixel each would be
    // needed for colour + gray; stage_in holds 6 bytes/pixel)
    rc = ingest(ctx, 0, left, w, h, channels, preprocessed, f.left, ctx->stage_in);
    if (rc) return rc;
    // the second ingest reuses the staging area: order on the stream makes that safe
    rc = ingest(ctx, 1, right, w, h, channels, preprocessed, f.right, ctx->stage_in);
    if (rc) return rc;
    f.w = w; f.h = h; f.has_pair = true; f.has_disp = false; f.has_kp = false; f.kp_depth = false; f.sp_pending = false; f.n_kp = 0; f.kp_pending = false;
    return VO_OK;
}

// one image into a slot (monocular front end, BASELINE config 5): same ingest as the left image of a pair
extern "C" int vo_upload_mono(vo_ctx* ctx, int slot, const uint8_t* img, int w, int h, int channels)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!img || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_upload_mono: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& f = ctx->slots[slot];
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;
    StageTimer t(ctx, VO_T_UPLOAD);
    if ((rc = ingest(ctx, 0, img, w, h, channels, 1, f.left, ctx->stage_in))) return rc;
    f.w = w; f.h = h; f.has_pair = true; f.has_disp = false; f.has_kp = false; f.kp_depth = false; f.sp_pending = false; f.n_kp = 0; f.kp_pending = false;
    return VO_OK;
}

// ---- inputs kept resident in HBM (streaming ingest / benchmarking) -----------------------
extern "C" int vo_stage_pairs_alloc(vo_ctx* ctx, int n, int w, int h, int channels)
{
    if (!ctx || n <= 0 || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_stage_pairs_alloc: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context", w, h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    // (an in-place pair's front reads the staged images: the fronts the open group still holds are launched before they go)
    if (int rc = sweep_group_flush_fronts(ctx, true)) return rc;
    if (ctx->staged) { (void)hipFree(ctx->staged); ctx->staged = nullptr; }
    ctx->staged_n = 0;
    const size_t per = (size_t)w * h * channels;
    VO_HIP(ctx, hipMalloc((void**)&ctx->staged, per * 2 * n));
    ctx->staged_n = n; ctx->staged_w = w; ctx->staged_h = h; ctx->staged_ch = channels;
    return VO_OK;
}

extern "C" int vo_stage_pair(vo_ctx* ctx, int index, const uint8_t* left, const uint8_t* right)
{
    if (!ctx || !left || !right || index < 0 || index >= ctx->staged_n) return vo_fail(ctx, VO_E_ARG, "vo_stage_pair: bad index");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)ctx->staged_w * ctx->staged_h * ctx->staged_ch;
    if (int rc = sweep_group_flush_fronts(ctx, true)) return rc;     // (a pending front may still have to read this pair)
    VO_HIP(ctx, hipMemcpyAsync(ctx->staged + per * 2 * index, left, per, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(ctx->staged + per * (2 * index + 1), right, per, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_load_staged_pair(vo_ctx* ctx, int slot, int index, int preprocessed)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (index < 0 || index >= ctx->staged_n) return vo_fail(ctx, VO_E_ARG, "vo_load_staged_pair: bad index");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& f = ctx->slots[slot];
    const int w = ctx->staged_w, h = ctx->staged_h;
    const size_t per = (size_t)w * h * ctx->staged_ch;
    StageTimer t(ctx, VO_T_UPLOAD);
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;
    rc = ingest(ctx, 0, ctx->staged + per * 2 * index, w, h, ctx->staged_ch, preprocessed, f.left, ctx->stage_in, hipMemcpyDeviceToDevice);
    if (rc) return rc;
    rc = ingest(ctx, 1, ctx->staged + per * (2 * index + 1), w, h, ctx->staged_ch, preprocessed, f.right, ctx->stage_in, hipMemcpyDeviceToDevice);
    if (rc) return rc;
    f.w = w; f.h = h; f.has_pair = true; f.has_disp = false; f.has_kp = false; f.kp_depth = false; f.sp_pending = false; f.n_kp = 0; f.kp_pending = false;
    return VO_OK;
}

// Retargets the context at a look-ahead engine for the lifetime of the object: its stream stands in for the main one, its staging
// buffer changes places with the main one, `ws` / `orbws` point at the engine's SGBM workspace (engine 0: the main one) and ORB scratch.  No member
// of any workspace is copied or swapped.  Whatever path leaves the scope -- a status funnelled through rc or an early return of
// a VO_HIP check added later -- the context comes back pointing at its own.
struct EngineScope {
    vo_ctx* ctx;
    int engine;
    hipStream_t stream0;
    EngineScope(vo_ctx* c, int e) : ctx(c), engine(e), stream0(c->stream)
    {
        ctx->stream = ctx->la_stream[engine];
        std::swap(ctx->stage_in, ctx->la_stage[engine]);
        ctx->ws = engine == 0 ? &ctx->main_ws : &ctx->ws_alt[engine];
        ctx->orbws = &ctx->ws_alt[engine].orb;
        ctx->cur_engine = engine;
    }
    ~EngineScope()
    {
        ctx->cur_engine = -1;
        ctx->ws = &ctx->main_ws;
        ctx->orbws = &ctx->main_ws.orb;
        std::swap(ctx->stage_in, ctx->la_stage[engine]);
        ctx->stream = stream0;
    }
    EngineScope(const EngineScope&) = delete;
    EngineScope& operator=(const EngineScope&) = delete;
};

// an engine's stream, events, staging and ORB scratch at its first use; its SGBM workspace (engines 1 ..: about 0.95 GB at 1280 x 720,
// D = 128) with them unless the caller is a SPARSE submission (want_sgbm = false): it then comes when the first dense pair or
// monocular extraction lands on the engine
static int engine_prepare(vo_ctx* ctx, int engine, bool want_sgbm)
{
    if (!ctx->la_stream[engine]) VO_HIP(ctx, hipStreamCreateWithFlags(&ctx->la_stream[engine], hipStreamNonBlocking));
    if (!ctx->ws_alt[engine].mid) {
        VO_HIP(ctx, hipEventCreateWithFlags(&ctx->ws_alt[engine].mid, hipEventDisableTiming));
        VO_HIP(ctx, hipEventCreateWithFlags(&ctx->ws_alt[engine].swept, hipEventDisableTiming));
        VO_HIP(ctx, hipEventCreateWithFlags(&ctx->ws_alt[engine].moved, hipEventDisableTiming));
    }
    if (!ctx->la_stage[engine]) {
        VO_HIP(ctx, hipMalloc((void**)&ctx->la_stage[engine], ctx->stage_bytes * 2 + 256));
        if (orb_ws_alloc(ctx, ctx->ws_alt[engine].orb)) return vo_fail(ctx, VO_E_HIP, "hipMalloc failed (look-ahead ORB workspace)");
    }
    if (!want_sgbm || engine == 0 || ctx->ws_alt[engine].ready) return VO_OK;
    const hipError_t e = sgbm_ws_alloc(ctx, ctx->ws_alt[engine]);
    if (e != hipSuccess) return vo_fail(ctx, VO_E_HIP, "look-ahead engine %d: workspace allocation failed: %s", engine, hipGetErrorString(e));
    return VO_OK;
}

int slot_wait(vo_ctx* ctx, FrameSlot& f)
{
    if (int rc = sweep_group_close_for(ctx, f)) return rc;       // (`ready` is recorded for this run only once its group has closed)
    if (f.pending) {
        VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, f.ready, 0));
        f.pending = false;
        if (f.counted && ctx->inflight > 0) ctx->inflight--;
        f.counted = false;
    }
    return VO_OK;
}

// the caller gives up a look-ahead slot without consuming it (a prediction that did not come true): its work may still be
// running -- the slot stays `pending` for ordering -- but it no longer counts as in flight
extern "C" int vo_lookahead_drop(vo_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS) return vo_fail(ctx, VO_E_ARG, "vo_lookahead_drop: bad slot");
    FrameSlot& f = ctx->slots[slot];
    if (int rc = sweep_group_close_for(ctx, f)) return rc;
    if (f.pending && f.counted && ctx->inflight > 0) ctx->inflight--;
    f.counted = false;
    return VO_OK;
}

int slot_before_overwrite(vo_ctx* ctx, FrameSlot& f)
{
    // an earlier look-ahead run into this slot that nobody waited for (a voided prediction) may still be writing it on
    // another engine's stream, and pose steps started ahead may still be reading it on theirs
    if (int rc = sweep_group_close_for(ctx, f)) return rc;
    if (f.pending) VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, f.ready, 0));
    for (hipEvent_t& r : f.readers)
        if (r) { VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, r, 0)); r = nullptr; }
    // ... and a monocular pose step may still be writing its depths; what the slot held is gone with the refill
    if (f.depth_writer) { VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, f.depth_writer, 0)); f.depth_writer = nullptr; }
    f.mono_serial = 0;
    return VO_OK;
}

// Registers the completion event of an asynchronous step that reads the slot.  The slot keeps two entries: an entry is free
// when it is empty or its event has completed; with both still open (a step begun on a slot while two earlier readers of
// it are unfinished) the older one is waited for here, on the host, rather than dropped from the set a refill orders
// itself behind.
void slot_add_reader(FrameSlot& f, hipEvent_t done)
{
    for (hipEvent_t r : f.readers) if (r == done) return;
    for (hipEvent_t& r : f.readers)
        if (!r || hipEventQuery(r) == hipSuccess) { r = done; return; }
    (void)hipEventSynchronize(f.readers[0]);
    f.readers[0] = f.readers[1];
    f.readers[1] = done;
}

// common tail of the look-ahead entry points: ingest (device or pinned-host source) + SGBM (+ ORB) of one
// pair on the next engine's stream, `ready` recorded at the end.  sp (the *_sparse entries): no SGBM -- behind the ingest the whole
// sparse stereo chain with that request, in the engine's own SparseWs (the engine's next pair reuses it before the host has read
// anything: what the host reads lies in the slot)
static int prefetch_pair(vo_ctx* ctx, int slot, const uint8_t* srcL, const uint8_t* srcR, bool from_host, int w, int h,
                         int channels, int preprocessed, vo_ctx::HostStage* hs = nullptr, const SparseReq* sp = nullptr)
{
    int rc;
    FrameSlot& f = ctx->slots[slot];
    const int engine = ctx->next_engine;
    if ((rc = engine_prepare(ctx, engine, sp == nullptr))) return rc;
    if (sp && (rc = sparse_ws_prepare(ctx, ctx->sp_alt[engine], ctx->la_stream[engine], true))) return rc;
    // an engine holds one member of the open group at a time (this pair's front would land on its stream ahead of that member's
    // back part and reuse its workspace), and a slot that is a member is not refilled before its run is complete
    if ((f.in_group || sweep_group_has_engine(ctx, engine)) && (rc = sweep_group_close(ctx, f.in_group ? VO_GRP_CONSUMER : VO_GRP_OTHER))) return rc;
    bool deferred = false;
    const size_t per = (size_t)w * h * channels;
    hipMemcpyKind kind = hipMemcpyDeviceToDevice;
    if (hs) {
        kind = hipMemcpyHostToDevice;                 // pinned staging filled ahead by vo_host_stage_pair
    } else if (from_host) {
        // user memory -> this engine's pinned buffer (plain memcpy) -> async H2D on the engine's stream;
        // the buffer is reused only after the previous copy out of it has finished
        vo_ctx::SgbmWs& a = ctx->ws_alt[engine];
        if (!a.pinned) {
            VO_HIP(ctx, hipHostMalloc((void**)&a.pinned, ctx->stage_bytes * 2, hipHostMallocDefault));
            VO_HIP(ctx, hipEventCreateWithFlags(&a.h2d_done, hipEventDisableTiming));
        }
        if (a.h2d_valid) VO_HIP(ctx, hipEventSynchronize(a.h2d_done));
        memcpy(a.pinned, srcL, per);
        memcpy(a.pinned + per, srcR, per);
        srcL = a.pinned; srcR = a.pinned + per;
        kind = hipMemcpyHostToDevice;
    }
    ctx->next_engine = (engine + 1) % ctx->n_engines;
    f.w = w; f.h = h; f.has_kp = false; f.kp_depth = false; f.sp_pending = false; f.sp_ahead = false; f.n_kp = 0; f.kp_pending = false;
    if (sp) { f.mono_serial = 0; f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1; }   // (as vo_sparse_stereo)
    {
        EngineScope on_engine(ctx, engine);          // ctx->stream / staging / SGBM + ORB workspaces are the engine's in here
        // a dense pair that may defer goes on the open group's lane while groups are in force (ingest, front, and the whole chain
        // where the geometry then keeps it from deferring), everything else on the engine's own stream
        hipStream_t const target = sp ? ctx->la_stream[engine] : dense_stream(ctx, engine);
        const bool on_lane = stream_is_lane(ctx, target);
        rc = engine_enter(ctx, engine, target);
        const int stagger = ctx->tune_stagger >= 0 ? ctx->tune_stagger : (7 * ctx->n_engines + 8) / 16;
        if (!sp && !on_lane && stagger > 0 && stagger < ctx->n_engines) {          // (the stagger spreads SGBM stages: a sparse pair has none; a lane is in order already)
            vo_ctx::SgbmWs& p = ctx->ws_alt[(engine - stagger + ctx->n_engines) % ctx->n_engines];
            if (p.mid_valid) (void)hipStreamWaitEvent(ctx->stream, p.mid, 0);
        }
        if (!rc) rc = slot_before_overwrite(ctx, f);
        // a rectified gray pair that already lies in HBM needs no ingest step of its own: the SGBM run's first kernel reads it
        // where it lies and leaves the slot's copy behind (two copy commands less per pair on the engine's queue)
        const bool in_place = !sp && kind == hipMemcpyDeviceToDevice && preprocessed && channels == 1;
        if (!rc && !in_place) {
            StageTimer t(ctx, VO_T_UPLOAD);
            const bool pinned_src = hs != nullptr || from_host;   // (the library's own pinned staging either way)
            rc = ingest(ctx, 0, srcL, w, h, channels, preprocessed, f.left, ctx->stage_in, kind, pinned_src);
            if (!rc) rc = ingest(ctx, 1, srcR, w, h, channels, preprocessed, f.right, ctx->stage_in, kind, pinned_src);
        }
        if (!rc && hs) {
            std::lock_guard<std::mutex> lk(ctx->stage_mu);
            if (hipEventRecord(hs->h2d_done, ctx->stream) == hipSuccess) hs->valid = true;
            else rc = vo_fail(ctx, VO_E_HIP, "hipEventRecord failed");
        } else if (!rc && from_host) {
            vo_ctx::SgbmWs& a = ctx->ws_alt[engine];
            if (hipEventRecord(a.h2d_done, ctx->stream) == hipSuccess) a.h2d_valid = true;
            else rc = vo_fail(ctx, VO_E_HIP, "hipEventRecord failed");
        }
#ifdef VO_TEST_HOOKS
        if (!rc && ctx->fault_prefetch > 0 && --ctx->fault_prefetch == 0)
            rc = vo_fail(ctx, VO_E_STATE, "injected failure (VO_FAULT_PREFETCH) inside the engine scope");
#endif
        if (!rc && sp) rc = sparse_enqueue(ctx, f, ctx->sp_alt[engine], *sp);
        else if (!rc) rc = in_place ? sgbm_run(ctx, f, w, h, srcL, srcR, &deferred) : sgbm_run(ctx, f, w, h, nullptr, nullptr, &deferred);
        if (!rc && !sp && !deferred && ctx->la_orb) {
            const int* q = ctx->la_orb_params;
            rc = orb_slot_enqueue(ctx, f, q[0], q[1], q[2], q[3]);
            if (!rc) { memcpy(f.kp_params, q, sizeof(f.kp_params)); f.kp_pending = true; }
        }
        if (!rc && !deferred && hipEventRecord(f.ready, ctx->stream) != hipSuccess) rc = vo_fail(ctx, VO_E_HIP, "hipEventRecord failed");
    }
    if (rc) {
        // the slot holds a half-processed pair: nothing in it may be handed out
        f.kp_pending = false; f.has_pair = false; f.has_disp = false;
        if (f.counted && ctx->inflight > 0) ctx->inflight--;
        f.counted = false;                               // (`pending` stays: an earlier run into this slot may still be in flight)
        return rc;
    }
    f.has_pair = true; f.has_disp = sp == nullptr;
    if (sp) { f.sp_req = *sp; f.sp_pending = true; }
    if (!f.counted) ctx->inflight++;
    f.pending = true; f.counted = true;
    // (a member of the open group: the sweep, the post filters, the ORB chain and `ready` follow when the group closes)
    if (deferred && sweep_group_members(ctx) >= sweep_group_size(ctx)) return sweep_group_close(ctx, VO_GRP_FULL);
    return VO_OK;
}

// look-ahead: ingest + SGBM of a staged pair on an engine's stream.  The main stream keeps running
// the current pair's ORB / matching / pose meanwhile; consumers of the slot wait for `ready`.
extern "C" int vo_prefetch_staged_pair(vo_ctx* ctx, int slot, int index, int preprocessed)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (index < 0 || index >= ctx->staged_n) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_staged_pair: bad index");
    if (!ctx->sg.set) return vo_fail(ctx, VO_E_STATE, "vo_set_sgbm has not been called");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)ctx->staged_w * ctx->staged_h * ctx->staged_ch;
    return prefetch_pair(ctx, slot, ctx->staged + per * 2 * index, ctx->staged + per * (2 * index + 1), false, ctx->staged_w,
                         ctx->staged_h, ctx->staged_ch, preprocessed);
}

// The three look-ahead entries with the sparse stereo chain in place of the SGBM (include/vo355.h): the request is checked before
// anything is enqueued; vo_set_Q is needed, vo_set_sgbm is not
static int host_stage_wait(vo_ctx* ctx, int buf);
static int sparse_entry_check(vo_ctx* ctx, const SparseReq& q, const char* who)
{
    if (int rc = sparse_req_check(ctx, q, who)) return rc;
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    return VO_OK;
}

extern "C" int vo_prefetch_staged_pair_sparse(vo_ctx* ctx, int slot, int index, int preprocessed, int nfeatures, float min_disp, float max_disp,
                                              float row_tol, int max_hamming)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (index < 0 || index >= ctx->staged_n) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_staged_pair_sparse: bad index");
    const SparseReq q = { nfeatures, min_disp, max_disp, row_tol, max_hamming, ctx->sp_assoc_flags, ctx->sp_assoc_ratio };
    if ((rc = sparse_entry_check(ctx, q, "vo_prefetch_staged_pair_sparse"))) return rc;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)ctx->staged_w * ctx->staged_h * ctx->staged_ch;
    return prefetch_pair(ctx, slot, ctx->staged + per * 2 * index, ctx->staged + per * (2 * index + 1), false, ctx->staged_w,
                         ctx->staged_h, ctx->staged_ch, preprocessed, nullptr, &q);
}

extern "C" int vo_prefetch_pair_sparse(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h, int channels,
                                       int preprocessed, int nfeatures, float min_disp, float max_disp, float row_tol, int max_hamming)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!left || !right || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_pair_sparse: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    const SparseReq q = { nfeatures, min_disp, max_disp, row_tol, max_hamming, ctx->sp_assoc_flags, ctx->sp_assoc_ratio };
    if ((rc = sparse_entry_check(ctx, q, "vo_prefetch_pair_sparse"))) return rc;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    return prefetch_pair(ctx, slot, left, right, true, w, h, channels, preprocessed, nullptr, &q);
}

extern "C" int vo_prefetch_host_staged_sparse(vo_ctx* ctx, int slot, int buf, int w, int h, int channels, int preprocessed, int nfeatures,
                                              float min_disp, float max_disp, float row_tol, int max_hamming)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (buf < 0 || buf >= vo_ctx::N_HOST_STAGE || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_host_staged_sparse: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    const SparseReq q = { nfeatures, min_disp, max_disp, row_tol, max_hamming, ctx->sp_assoc_flags, ctx->sp_assoc_ratio };
    if ((rc = sparse_entry_check(ctx, q, "vo_prefetch_host_staged_sparse"))) return rc;
    vo_ctx::HostStage& hs = ctx->host_stage[buf];
    if (!hs.pinned) return vo_fail(ctx, VO_E_STATE, "staging buffer %d has not been filled (vo_host_stage_pair / vo_host_stage_begin)", buf);
    if ((rc = host_stage_wait(ctx, buf))) return vo_fail(ctx, rc, "the copy into staging buffer %d failed", buf);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)w * h * channels;
    return prefetch_pair(ctx, slot, hs.pinned, hs.pinned + per, true, w, h, channels, preprocessed, &hs, &q);
}

// monocular look-ahead (config 5): the left image of a staged pair into a slot and its ORB extraction (no disparity
// mask), all on a look-ahead engine's stream; vo_orb_detect_and_compute with the same nfeatures / mask_mode 0 then only
// waits.  The main stream keeps matching and scoring the previous pair meanwhile.
extern "C" int vo_prefetch_staged_mono(vo_ctx* ctx, int slot, int index, int nfeatures)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (index < 0 || index >= ctx->staged_n) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_staged_mono: bad index");
    if (nfeatures < 0 || nfeatures > ctx->max_kp) return vo_fail(ctx, VO_E_CAP, "nfeatures %d exceeds max_kp %d", nfeatures, ctx->max_kp);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& f = ctx->slots[slot];
    // a monocular extraction is short: four engines cover any useful look-ahead (an engine's first use allocates its workspaces)
    const int span = ctx->n_engines < 4 ? ctx->n_engines : 4;
    const int engine = ctx->mono_engine % span;
    if ((rc = engine_prepare(ctx, engine, true))) return rc;      // (as ever on this path: the engine's workspaces all come with its first use)
    if ((f.in_group || sweep_group_has_engine(ctx, engine)) && (rc = sweep_group_close(ctx, f.in_group ? VO_GRP_CONSUMER : VO_GRP_OTHER))) return rc;
    ctx->mono_engine = (engine + 1) % span;
    const size_t per = (size_t)ctx->staged_w * ctx->staged_h * ctx->staged_ch;
    const int w = ctx->staged_w, h = ctx->staged_h;
    f.w = w; f.h = h; f.has_kp = false; f.kp_depth = false; f.sp_pending = false; f.n_kp = 0; f.kp_pending = false; f.has_disp = false;
    {
        EngineScope on_engine(ctx, engine);
        rc = engine_enter(ctx, engine, ctx->la_stream[engine]);   // (the engine's ORB scratch may still serve the group it was last a member of)
        if (!rc) rc = slot_before_overwrite(ctx, f);
        if (!rc) {
            StageTimer t(ctx, VO_T_UPLOAD);
            rc = ingest(ctx, 0, ctx->staged + per * 2 * index, w, h, ctx->staged_ch, 1, f.left, ctx->stage_in, hipMemcpyDeviceToDevice);
        }
        const int params[4] = { nfeatures, 0, 0, 0 };
        if (!rc) rc = orb_slot_enqueue(ctx, f, nfeatures, 0, 0, 0);
        if (!rc) { memcpy(f.kp_params, params, sizeof(f.kp_params)); f.kp_pending = true; }
        if (!rc && hipEventRecord(f.ready, ctx->stream) != hipSuccess) rc = vo_fail(ctx, VO_E_HIP, "hipEventRecord failed");
    }
    if (rc) {
        f.kp_pending = false; f.has_pair = false;
        if (f.counted && ctx->inflight > 0) ctx->inflight--;
        f.counted = false;
        return rc;
    }
    f.has_pair = true;
    if (!f.counted) ctx->inflight++;
    f.pending = true; f.counted = true;
    return VO_OK;
}

// the same from host images (the user's decode/ingest step): the upload of pair i+k overlaps the work
// on pair i; the host buffers are free again when the call returns
extern "C" int vo_prefetch_pair(vo_ctx* ctx, int slot, const uint8_t* left, const uint8_t* right, int w, int h, int channels,
                                int preprocessed)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!left || !right || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_pair: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    if (!ctx->sg.set) return vo_fail(ctx, VO_E_STATE, "vo_set_sgbm has not been called");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    return prefetch_pair(ctx, slot, left, right, true, w, h, channels, preprocessed);
}

static int host_stage_alloc(vo_ctx* ctx)
{
    // first use of the staging path: every buffer at once (a pinned allocation takes about a millisecond -- not something to
    // pay inside a stream, buffer by buffer).  Under the staging lock: vo_host_stage_pair may run on a helper thread of the
    // caller while the driving thread calls vo_host_stage_begin.
    std::lock_guard<std::mutex> lk(ctx->stage_mu);
    for (vo_ctx::HostStage& q : ctx->host_stage) {
        if (q.pinned) continue;
        if (hipHostMalloc((void**)&q.pinned, ctx->stage_bytes * 2, hipHostMallocDefault) != hipSuccess) return VO_E_HIP;
        if (hipEventCreateWithFlags(&q.h2d_done, hipEventDisableTiming) != hipSuccess) return VO_E_HIP;
    }
    return VO_OK;
}

// body of the staging thread: one copy at a time, in the order asked for
static void host_stage_loop(vo_ctx* ctx)
{
    (void)hipSetDevice(ctx->device);
    for (;;) {
        vo_ctx::StageJob job;
        hipEvent_t wait_for = nullptr;
        {
            std::unique_lock<std::mutex> lk(ctx->stage_mu);
            ctx->stage_cv.wait(lk, [&] { return ctx->stage_stop || !ctx->stage_jobs.empty(); });
            if (ctx->stage_stop) return;
            job = ctx->stage_jobs.front();
            ctx->stage_jobs.pop_front();
            vo_ctx::HostStage& hs = ctx->host_stage[job.buf];
            if (hs.valid) wait_for = hs.h2d_done;     // the previous upload out of this buffer
        }
        int rc = VO_OK;
        if (wait_for && hipEventSynchronize(wait_for) != hipSuccess) rc = VO_E_HIP;
        if (!rc) {
            vo_ctx::HostStage& hs = ctx->host_stage[job.buf];
            memcpy(hs.pinned, job.left, job.per);
            memcpy(hs.pinned + job.per, job.right, job.per);
        }
        {
            std::lock_guard<std::mutex> lk(ctx->stage_mu);
            ctx->host_stage[job.buf].state = rc;
        }
        ctx->stage_cv.notify_all();
    }
}

// until the copy begun into `buf` has finished (at once when none is pending); its status
static int host_stage_wait(vo_ctx* ctx, int buf)
{
    std::unique_lock<std::mutex> lk(ctx->stage_mu);
    vo_ctx::HostStage& hs = ctx->host_stage[buf];
    ctx->stage_cv.wait(lk, [&] { return hs.state != 1; });
    const int rc = hs.state;
    hs.state = 0;
    return rc;
}

// The copy of a host pair into pinned staging buffer `buf`, handed to the library's staging thread: returns at once.  The two
// images must stay untouched until vo_host_stage_wait / vo_prefetch_host_staged / vo_host_stage_fetch on that buffer returns.
extern "C" int vo_host_stage_begin(vo_ctx* ctx, int buf, const uint8_t* left, const uint8_t* right, int w, int h, int channels)
{
    if (!ctx || buf < 0 || buf >= vo_ctx::N_HOST_STAGE || !left || !right || (channels != 1 && channels != 3))
        return vo_fail(ctx, VO_E_ARG, "vo_host_stage_begin: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (host_stage_alloc(ctx)) return vo_fail(ctx, VO_E_HIP, "pinned staging memory: allocation failed");
    {
        std::lock_guard<std::mutex> lk(ctx->stage_mu);
        vo_ctx::HostStage& hs = ctx->host_stage[buf];
        if (hs.state == 1) return vo_fail(ctx, VO_E_STATE, "vo_host_stage_begin: a copy into buffer %d is still pending", buf);
        hs.state = 1;
        ctx->stage_jobs.push_back({ buf, left, right, (size_t)w * h * channels });
        if (!ctx->stage_thread.joinable()) ctx->stage_thread = std::thread(host_stage_loop, ctx);
    }
    ctx->stage_cv.notify_all();
    return VO_OK;
}

extern "C" int vo_host_stage_wait(vo_ctx* ctx, int buf)
{
    if (!ctx || buf < 0 || buf >= vo_ctx::N_HOST_STAGE) return vo_fail(ctx, VO_E_ARG, "vo_host_stage_wait: bad argument");
    const int rc = host_stage_wait(ctx, buf);
    return rc ? vo_fail(ctx, rc, "the copy into staging buffer %d failed", buf) : VO_OK;
}

// The same copy done by the calling thread.  May run on a helper thread of the caller while another thread drives the
// context: it touches nothing but staging buffer `buf` (and reports failures by code only: the context's error string
// belongs to the driving thread).
extern "C" int vo_host_stage_pair(vo_ctx* ctx, int buf, const uint8_t* left, const uint8_t* right, int w, int h, int channels)
{
    if (!ctx || buf < 0 || buf >= vo_ctx::N_HOST_STAGE || !left || !right || (channels != 1 && channels != 3)) return VO_E_ARG;
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return VO_E_CAP;
    if (hipSetDevice(ctx->device) != hipSuccess) return VO_E_HIP;
    if (host_stage_alloc(ctx)) return VO_E_HIP;
    if (int rcw = host_stage_wait(ctx, buf)) return rcw;
    vo_ctx::HostStage& hs = ctx->host_stage[buf];
    hipEvent_t wait_for = nullptr;
    { std::lock_guard<std::mutex> lk(ctx->stage_mu); if (hs.valid) wait_for = hs.h2d_done; }
    if (wait_for && hipEventSynchronize(wait_for) != hipSuccess) return VO_E_HIP;   // the previous upload out of this buffer
    const size_t per = (size_t)w * h * channels;
    memcpy(hs.pinned, left, per);
    memcpy(hs.pinned + per, right, per);
    return VO_OK;
}

// the pair a staging buffer holds, copied back out (the caller found no free slot for it and keeps it on the host)
extern "C" int vo_host_stage_fetch(vo_ctx* ctx, int buf, uint8_t* left, uint8_t* right, int w, int h, int channels)
{
    if (!ctx || buf < 0 || buf >= vo_ctx::N_HOST_STAGE || !left || !right || (channels != 1 && channels != 3)) return VO_E_ARG;
    vo_ctx::HostStage& hs = ctx->host_stage[buf];
    if (!hs.pinned || (size_t)w * h * channels > ctx->stage_bytes) return VO_E_STATE;
    if (int rcw = host_stage_wait(ctx, buf)) return rcw;
    const size_t per = (size_t)w * h * channels;
    memcpy(left, hs.pinned, per);
    memcpy(right, hs.pinned + per, per);
    return VO_OK;
}

extern "C" int vo_prefetch_host_staged(vo_ctx* ctx, int slot, int buf, int w, int h, int channels, int preprocessed)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (buf < 0 || buf >= vo_ctx::N_HOST_STAGE || (channels != 1 && channels != 3)) return vo_fail(ctx, VO_E_ARG, "vo_prefetch_host_staged: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    if (!ctx->sg.set) return vo_fail(ctx, VO_E_STATE, "vo_set_sgbm has not been called");
    vo_ctx::HostStage& hs = ctx->host_stage[buf];
    if (!hs.pinned) return vo_fail(ctx, VO_E_STATE, "staging buffer %d has not been filled (vo_host_stage_pair / vo_host_stage_begin)", buf);
    if ((rc = host_stage_wait(ctx, buf))) return vo_fail(ctx, rc, "the copy into staging buffer %d failed", buf);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)w * h * channels;
    return prefetch_pair(ctx, slot, hs.pinned, hs.pinned + per, true, w, h, channels, preprocessed, &hs);
}

extern "C" int vo_set_lookahead_orb(vo_ctx* ctx, int enable, int nfeatures, int mask_mode, int min_disp16, int max_disp16)
{
    if (!ctx) return VO_E_ARG;
    if (enable) {
        if (nfeatures < 0 || nfeatures > ctx->max_kp) return vo_fail(ctx, VO_E_CAP, "nfeatures %d exceeds max_kp %d", nfeatures, ctx->max_kp);
        if (mask_mode != 0 && mask_mode != 1) return vo_fail(ctx, VO_E_ARG, "mask_mode must be 0 or 1");
    }
    if (int rc = sweep_group_close(ctx, VO_GRP_OTHER)) return rc;     // its members' ORB chains run with the parameters they were submitted under
    ctx->la_orb = enable != 0;
    ctx->la_orb_params[0] = nfeatures; ctx->la_orb_params[1] = mask_mode;
    ctx->la_orb_params[2] = min_disp16; ctx->la_orb_params[3] = max_disp16;
    return VO_OK;
}

extern "C" int vo_sgbm_compute(vo_ctx* ctx, int slot, int16_t* disp16_out)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_pair) return vo_fail(ctx, VO_E_STATE, "slot %d holds no image pair", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = slot_wait(ctx, f))) return rc;
    rc = sgbm_run(ctx, f, f.w, f.h);
    if (rc) return rc;
    f.has_disp = true; f.kp_pending = false; f.has_kp = false; f.kp_depth = false; f.sp_pending = false;
    if (disp16_out) {
        VO_HIP(ctx, hipMemcpyAsync(disp16_out, f.disp16, (size_t)f.w * f.h * 2, hipMemcpyDeviceToHost, ctx->stream));
        VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return slot_health(ctx, f, slot);
    }
    return VO_OK;
}

extern "C" int vo_sgbm_compute_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int16_t* disp16_out)
{
    if (!ctx || !left || !right || !disp16_out) return vo_fail(ctx, VO_E_ARG, "vo_sgbm_compute_host: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context", w, h);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& f = ctx->slots[VO_NUM_SLOTS];
    VO_HIP(ctx, hipMemcpyAsync(f.left, left, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(f.right, right, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream));
    int rc = sgbm_run(ctx, f, w, h);
    if (rc) return rc;
    VO_HIP(ctx, hipMemcpyAsync(disp16_out, f.disp16, (size_t)w * h * 2, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return slot_health(ctx, f, VO_NUM_SLOTS);
}

extern "C" int vo_cvt_bgr2gray(vo_ctx* ctx, const uint8_t* bgr, int w, int h, uint8_t* gray)
{
    if (!ctx || !bgr || !gray) return vo_fail(ctx, VO_E_ARG, "vo_cvt_bgr2gray: bad argument");
    if ((size_t)w * h > (size_t)ctx->max_w * ctx->max_h) return vo_fail(ctx, VO_E_CAP, "image too large");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)w * h;
    VO_HIP(ctx, hipMemcpyAsync(ctx->stage_in, bgr, n * 3, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_bgr2gray, dim3(div_up((int)n, 256)), dim3(256), 0, ctx->stream, ctx->stage_in, (int)n, ctx->stage_in + n * 3);
    VO_CHECK_LAUNCH(ctx);
    VO_HIP(ctx, hipMemcpyAsync(gray, ctx->stage_in + n * 3, n, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_remap(vo_ctx* ctx, int cam, const uint8_t* src, int w, int h, uint8_t* dst)
{
    if (!ctx || !src || !dst || cam < 0 || cam > 1) return vo_fail(ctx, VO_E_ARG, "vo_remap: bad argument");
    if (!ctx->has_map[cam]) return vo_fail(ctx, VO_E_STATE, "maps of camera %d not set", cam);
    if ((size_t)w * h > (size_t)ctx->max_w * ctx->max_h) return vo_fail(ctx, VO_E_CAP, "image too large");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)w * h, nm = (size_t)ctx->map_w * ctx->map_h;
    VO_HIP(ctx, hipMemcpyAsync(ctx->stage_in, src, n, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* out = ctx->stage_in + ctx->stage_bytes;
    hipLaunchKernelGGL(k_remap, dim3(div_up(ctx->map_w, 256), ctx->map_h), dim3(256), 0, ctx->stream, ctx->stage_in, w, h,
                       ctx->map1[cam], ctx->map2[cam], ctx->map_w, ctx->map_h, out);
    VO_CHECK_LAUNCH(ctx);
    VO_HIP(ctx, hipMemcpyAsync(dst, out, nm, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

// ---- lazy downloads ---------------------------------------------------------------------
__global__ void k_disp_to_f32(const int16_t* __restrict__ d, int n, float* __restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)d[i] / 16.0f;
}

static int ensure_img3(vo_ctx* ctx, size_t bytes)
{
    if (ctx->img3_ws_bytes >= bytes) return VO_OK;
    if (ctx->img3_ws) (void)hipFree(ctx->img3_ws);
    ctx->img3_ws = nullptr; ctx->img3_ws_bytes = 0;
    VO_HIP(ctx, hipMalloc((void**)&ctx->img3_ws, bytes));
    ctx->img3_ws_bytes = bytes;
    return VO_OK;
}

extern "C" int vo_download_disparity_f32(vo_ctx* ctx, int slot, float* out)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_disp || !out) return vo_fail(ctx, VO_E_STATE, "slot %d holds no disparity", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = slot_wait(ctx, f))) return rc;
    const int n = f.w * f.h;
    if ((rc = ensure_img3(ctx, (size_t)n * 12))) return rc;
    hipLaunchKernelGGL(k_disp_to_f32, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, f.disp16, n, ctx->img3_ws);
    VO_CHECK_LAUNCH(ctx);
    VO_HIP(ctx, hipMemcpyAsync(out, ctx->img3_ws, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return slot_health(ctx, f, slot);
}

extern "C" int vo_download_left(vo_ctx* ctx, int slot, uint8_t* out)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_pair || !out) return vo_fail(ctx, VO_E_STATE, "slot %d holds no image", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = slot_wait(ctx, f))) return rc;
    VO_HIP(ctx, hipMemcpyAsync(out, f.left, (size_t)f.w * f.h, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_download_right(vo_ctx* ctx, int slot, uint8_t* out)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_pair || !out) return vo_fail(ctx, VO_E_STATE, "slot %d holds no image", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = slot_wait(ctx, f))) return rc;
    VO_HIP(ctx, hipMemcpyAsync(out, f.right, (size_t)f.w * f.h, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_slot_num_keypoints(vo_ctx* ctx, int slot, int* n_out)
{
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_out) return VO_E_ARG;
    *n_out = ctx->slots[slot].has_kp ? ctx->slots[slot].n_kp : 0;
    return VO_OK;
}

extern "C" int vo_enable_timing(vo_ctx* ctx, int on)
{
    if (!ctx) return VO_E_ARG;
    // on = 1: every stage; on > 1: bit mask (1 << stage) << 1 of the stages to time; 0: off
    ctx->timing = on != 0;
    ctx->timing_mask = on == 1 ? ~0u : (unsigned)on >> 1;
    return VO_OK;
}

// resolve the event pairs recorded so far (events are recorded without blocking the stream)
static void resolve_events(vo_ctx* ctx)
{
    if (ctx->ev_used == 0) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (size_t i = 0; i < ctx->ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->ev_pool[2 * i], ctx->ev_pool[2 * i + 1]) == hipSuccess) {
            ctx->t_ms[ctx->ev_stage[i]] += ms;
            ctx->t_n[ctx->ev_stage[i]] += ctx->ev_entries[i];
        }
    }
    ctx->ev_used = 0;
}

StageTimer::StageTimer(vo_ctx* ctx, int s, int entries) : c(ctx), stage(s), idx(-1)
{
    if (!c->timing || !((c->timing_mask >> s) & 1u) || entries <= 0) return;
    if (c->ev_used * 2 + 2 > c->ev_pool.size()) {
        if (c->ev_pool.size() >= 32768) resolve_events(c);
        else
            for (int k = 0; k < 512; k++) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) c->ev_pool.push_back(e); }
    }
    if (c->ev_used * 2 + 2 > c->ev_pool.size()) return;
    idx = (long)c->ev_used++;
    if (c->ev_stage.size() <= (size_t)idx) { c->ev_stage.resize(idx + 1); c->ev_entries.resize(idx + 1); }
    c->ev_stage[idx] = s;
    c->ev_entries[idx] = entries;
    (void)hipEventRecord(c->ev_pool[2 * idx], c->stream);
}
StageTimer::~StageTimer()
{
    if (idx >= 0) (void)hipEventRecord(c->ev_pool[2 * idx + 1], c->stream);
}

extern "C" int vo_get_timings(vo_ctx* ctx, double* ms_out, int64_t* launches_out, int reset)
{
    if (!ctx) return VO_E_ARG;
    resolve_events(ctx);
    for (int i = 0; i < VO_T_NSTAGES; i++) {
        if (ms_out) ms_out[i] = ctx->t_ms[i];
        if (launches_out) launches_out[i] = ctx->t_n[i];
        if (reset) { ctx->t_ms[i] = 0; ctx->t_n[i] = 0; }
    }
    return VO_OK;
}

extern "C" int vo_get_stage_timeline(vo_ctx* ctx, int cap, int32_t* stage_out, int32_t* entries_out, double* begin_ms_out, double* end_ms_out, int* n_out)
{
    if (!ctx || !n_out || cap < 0 || (cap > 0 && (!stage_out || !entries_out || !begin_ms_out || !end_ms_out)))
        return vo_fail(ctx, VO_E_ARG, "vo_get_stage_timeline: bad argument");
    *n_out = 0;
    if (ctx->ev_used == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    // brackets lie on the engines' and the pose steps' streams as well (the open sweep group, if any, stays open: its
    // members' fronts are complete brackets, the rest has not been recorded yet)
    VO_HIP(ctx, engine_streams_sync(ctx));
    for (int kind : { vo_ctx::ALT_POSE, vo_ctx::ALT_MONO })
        for (int k = 0; k < vo_ctx::alt_count(kind); k++)
            if (ctx->alt(kind, k).stream) VO_HIP(ctx, hipStreamSynchronize(ctx->alt(kind, k).stream));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (size_t i = 0; i < ctx->ev_used; i++) {
        float t0 = 0, dt = 0;
        if (hipEventElapsedTime(&t0, ctx->ev_pool[0], ctx->ev_pool[2 * i]) != hipSuccess ||
            hipEventElapsedTime(&dt, ctx->ev_pool[2 * i], ctx->ev_pool[2 * i + 1]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        if (n < cap) { stage_out[n] = ctx->ev_stage[i]; entries_out[n] = ctx->ev_entries[i]; begin_ms_out[n] = t0; end_ms_out[n] = (double)t0 + (double)dt; }
        n++;
    }
    *n_out = n;
    return VO_OK;
}

// the disparity a slot holds comes from a run whose diagonal sweep gave up a strip hand-off (see FrameSlot::sweep_word)
int slot_health(vo_ctx* ctx, const FrameSlot& f, int slot)
{
    if (f.disp_gen != 0 && f.sweep_word && *(volatile int32_t*)f.sweep_word == f.disp_gen)
        return vo_fail(ctx, VO_E_SWEEP, "slot %d: a strip hand-off of this pair's aggregation sweep gave up waiting (GPU oversubscribed?): "
                                        "its disparity is undefined and nothing computed from it is handed out; submit the pair again", slot);
    return VO_OK;
}

extern "C" int vo_sgbm_sweep_status(vo_ctx* ctx, int* error_out)
{
    if (!ctx || !error_out) return VO_E_ARG;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = vo_synchronize(ctx);
    if (rc) return rc;
    // SGBM runs of this context in which a wait inside a diagonal sweep exceeded its poll limit (counted by k_sgbm_fin)
    int n = 0;
    VO_HIP(ctx, hipMemcpy(&n, ctx->d_sweep_errs, sizeof(int), hipMemcpyDeviceToHost));
    *error_out = n;
    return VO_OK;
}

// ---- the box's streaming-copy ceiling (the HBM roofline is reported against the 8 TB/s peak and against
// what a plain device copy reaches on this very GPU) -------------------------------------------------------------
typedef uint32_t copy_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ void __launch_bounds__(256) k_copy_stream(const copy_u32x4* __restrict__ src, copy_u32x4* __restrict__ dst, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        if (NT) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
        else dst[i] = src[i];
    }
}

extern "C" int vo_measure_copy(vo_ctx* ctx, int64_t bytes, int reps, int nontemporal, double* gb_per_s)
{
    if (!ctx || !gb_per_s || reps <= 0) return vo_fail(ctx, VO_E_ARG, "vo_measure_copy: bad argument");
    // source = the first path volume, destination = the cost volume: both exist, neither holds anything a later call needs
    const int64_t cap = (int64_t)ctx->vol_cells * 2;
    if (bytes <= 0 || bytes > cap) bytes = cap;
    bytes &= ~(int64_t)4095;
    if (bytes <= 0 || !ctx->ws->C || !ctx->ws->S) return vo_fail(ctx, VO_E_STATE, "vo_measure_copy: no volumes to copy between");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    // the volumes belong to the main workspace (engine 0 uses it too): nothing of the pipeline may still be running
    ctx->c_last.valid = false;                              // (the copy lands in the cost volume)
    VO_HIP(ctx, engine_streams_sync(ctx));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hipEvent_t e0, e1;
    VO_HIP(ctx, hipEventCreate(&e0));
    VO_HIP(ctx, hipEventCreate(&e1));
    const size_t n16 = (size_t)bytes / 16;
    const int blocks = 256 * 16;                           // 16 workgroups per CU, grid-stride
    auto kern = nontemporal ? k_copy_stream<true> : k_copy_stream<false>;
    auto launch = [&]() { hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, ctx->stream, (const copy_u32x4*)ctx->ws->S, (copy_u32x4*)ctx->ws->C, n16); };
    launch();                                               // warm-up (page tables, clocks)
    VO_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; r++) launch();
    VO_HIP(ctx, hipEventRecord(e1, ctx->stream));
    VO_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    VO_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gb_per_s = ms > 0.f ? 2.0 * (double)bytes * reps / (ms * 1e-3) / 1e9 : 0.0;   // bytes read + bytes written
    return VO_OK;
}

__global__ void k_clock_probe(unsigned long long* out, unsigned long long ticks)
{
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long w = w0;
    unsigned v = threadIdx.x;
    while (w - w0 < ticks) {
#pragma unroll
        for (int i = 0; i < 64; i++) asm volatile("v_pk_add_i16 %0, %0, %0" : "+v"(v));
        w = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = w - w0; out[2] = v; }
}

extern "C" int vo_shader_clock(vo_ctx* ctx, int micros, double* mhz)
{
    if (!ctx || !mhz || micros <= 0 || micros > 1000000) return vo_fail(ctx, VO_E_ARG, "vo_shader_clock: bad argument");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long* d = (unsigned long long*)ctx->red;              // (reduction scratch: nothing of the pipeline keeps state in it)
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, ctx->stream, d, (unsigned long long)micros * 100ull);
    VO_CHECK_LAUNCH(ctx);
    unsigned long long h[2] = { 0, 0 };
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VO_HIP(ctx, hipMemcpy(h, d, 16, hipMemcpyDeviceToHost));
    *mhz = h[1] ? (double)h[0] / ((double)h[1] / 100.0) : 0.0;           // cycles per microsecond
    return VO_OK;
}

// timeline of the latest diagonal sweep in the main workspace (development aid): words [8 + 8 s ..] of control block `block`
// = {start, end, failed polls, ticks waiting, misses} of strip s in 100 MHz ticks
extern "C" int vo_sgbm_sweep_stats(vo_ctx* ctx, int block, int32_t* out, int n_words)
{
    if (!ctx || !out || block < 0 || block > 1 || n_words <= 0) return vo_fail(ctx, VO_E_ARG, "vo_sgbm_sweep_stats: bad argument");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = vo_synchronize(ctx);
    if (rc) return rc;
    const int half = ctx->sw_ctl_words / 2;
    if (n_words > half) n_words = half;
    VO_HIP(ctx, hipMemcpy(out, ctx->ws->sw_ctl + block * half, (size_t)n_words * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VO_OK;
}

// look-ahead pairs submitted and not yet waited for or dropped (what a per-pair scheduling policy would look at)
extern "C" int vo_lookahead_depth(vo_ctx* ctx, int* depth_out)
{
    if (!ctx || !depth_out) return VO_E_ARG;
    *depth_out = ctx->inflight;
    return VO_OK;
}

// has the look-ahead work into this slot finished?  (never blocks: a caller that runs ahead speculatively only picks up what is there)
extern "C" int vo_slot_ready(vo_ctx* ctx, int slot, int* ready_out)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || !ready_out) return vo_fail(ctx, VO_E_ARG, "vo_slot_ready: bad argument");
    FrameSlot& f = ctx->slots[slot];
    *ready_out = 1;
    if (int rc = sweep_group_close_for(ctx, f)) return rc;           // (enqueues the rest of the slot's run: still no wait)
    if (f.pending) {
        const hipError_t e = hipEventQuery(f.ready);
        if (e == hipErrorNotReady) *ready_out = 0;
        else if (e != hipSuccess) return vo_fail(ctx, VO_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
    }
    return VO_OK;
}

// which schedule the latest SGBM run of this context took (VO_SCHED_*)
extern "C" int vo_sgbm_last_schedule(vo_ctx* ctx, int* schedule_out)
{
    if (!ctx || !schedule_out) return VO_E_ARG;
    *schedule_out = ctx->last_schedule;
    return VO_OK;
}

extern "C" int vo_sgbm_last_geometry(vo_ctx* ctx, int64_t* cells, int* n_paths)
{
    if (!ctx) return VO_E_ARG;
    if (cells) *cells = ctx->last_cells;
    if (n_paths) *n_paths = ctx->last_paths;
    return VO_OK;
}

#ifdef VO_TEST_HOOKS
// Test-only build (libvo355_hooks.so): n keypoints with their descriptors and 3-D points written straight into a slot, which then
// stands exactly as vo_sparse_stereo leaves it (keypoints that carry depth; nothing pending, begun ahead or monocular).  The seam
// through which the tests drive the fused pose and PnP steps at chosen (nq, M) instead of what ORB finds in an image.  xy (n, 2)
// float32, desc (n, 32), xyz (n, 3) float32, rdesc (n, 32) or null (then zeros); size / angle / response / octave / disparity read 0.
extern "C" int vo_test_plant_keypoints(vo_ctx* ctx, int slot, int n, const float* xy, const uint8_t* desc, const float* xyz, const uint8_t* rdesc)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || n < 0) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_keypoints: bad argument");
    if (n > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "vo_test_plant_keypoints: %d keypoints exceed capacity %d", n, ctx->kp_cap);
    if (n > 0 && (!xy || !desc || !xyz)) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_keypoints: null pointer");
    FrameSlot& f = ctx->slots[slot];
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;     // (as vo_sparse_stereo: steps begun ahead may still read the slot)
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false; f.sp_pending = false; f.sp_ahead = false;
    f.mono_serial = 0;
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;
    f.sp_req.nfeatures = -1;                 // no request ever equals it: vo_sparse_stereo on this slot recomputes
    if ((rc = xfer_h2d(ctx, f.kp_xy, xy, (size_t)n * 8))) return rc;
    if ((rc = xfer_h2d(ctx, f.desc, desc, (size_t)n * 32))) return rc;
    if ((rc = xfer_h2d(ctx, f.kp_xyz, xyz, (size_t)n * 12))) return rc;
    if (rdesc) { if ((rc = xfer_h2d(ctx, f.kp_rdesc, rdesc, (size_t)n * 32))) return rc; }
    else if (n > 0) VO_HIP(ctx, hipMemsetAsync(f.kp_rdesc, 0, (size_t)n * 32, ctx->stream));
    if (n > 0) {
        VO_HIP(ctx, hipMemsetAsync(f.kp_size, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_angle, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_resp, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_oct, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_disp, 0, (size_t)n * 4, ctx->stream));
    }
    if ((rc = xfer_flush(ctx))) return rc;
    f.sp_rec[0] = f.sp_rec[1] = f.sp_rec[2] = f.sp_rec[3] = n;
    *f.n_kp_host = n;
    f.n_kp = n;
    f.has_kp = true; f.kp_depth = true;
    return VO_OK;
}

// ... and a DENSE slot: a w x h disparity image (int16, 1/16 px) and n keypoints with their descriptors, after which the slot stands
// as a synchronous vo_sgbm_compute followed by an ORB extraction leaves it (a disparity of a fresh, healthy generation; keypoints
// that carry NO depth) -- the seam through which the tests drive the bilinear lookup of vo_points3d_at / vo_point_clouds and the
// dense arm of the fused pose and PnP steps.  disp16 (h, w) int16, xy (n, 2) float32, desc (n, 32).  Everything is validated BEFORE
// the slot is touched: the kernels trust a keypoint to lie inside the crop under the ROI in force (as ORB's do), so a position
// outside it is refused here with the condition vo_points3d_at checks on the host -- set Q and the ROI first, and keep the ROI.
extern "C" int vo_test_plant_dense(vo_ctx* ctx, int slot, int w, int h, const int16_t* disp16, int n, const float* xy, const uint8_t* desc)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || n < 0) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_dense: bad argument");
    if (w > ctx->max_w || h > ctx->max_h || w < 16 || h < 16) return vo_fail(ctx, VO_E_CAP, "vo_test_plant_dense: image %dx%d exceeds context %dx%d", w, h, ctx->max_w, ctx->max_h);
    if (n > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "vo_test_plant_dense: %d keypoints exceed capacity %d", n, ctx->kp_cap);
    if (!disp16 || (n > 0 && (!xy || !desc))) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_dense: null pointer");
    const int cw = ctx->has_roi ? (ctx->roi[2] < w ? ctx->roi[2] : w) - ctx->roi[0] : w;
    const int ch = ctx->has_roi ? (ctx->roi[3] < h ? ctx->roi[3] : h) - ctx->roi[1] : h;
    if (cw <= 0 || ch <= 0) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_dense: the ROI leaves nothing of a %dx%d image", w, h);
    for (int i = 0; i < n; i++)      // (compared as floats: for 0 <= x that is (int)x < cw, and it also holds for inf and for values no int holds)
        if (!(xy[2 * i] >= 0 && xy[2 * i + 1] >= 0 && xy[2 * i] < (float)cw && xy[2 * i + 1] < (float)ch))
            return vo_fail(ctx, VO_E_ARG, "vo_test_plant_dense: keypoint %d (%g,%g) outside the %dx%d cropped image", i, xy[2 * i], xy[2 * i + 1], cw, ch);
    FrameSlot& f = ctx->slots[slot];
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;     // (steps begun ahead may still read the slot)
    f.has_pair = false; f.has_disp = false;      // (the images the slot may hold belong to another disparity: nothing recomputes from them)
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false; f.sp_pending = false; f.sp_ahead = false;
    f.mono_serial = 0;
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;
    f.sp_req.nfeatures = -1;
    if ((rc = xfer_h2d(ctx, f.disp16, disp16, (size_t)w * h * 2))) return rc;
    if ((rc = xfer_h2d(ctx, f.kp_xy, xy, (size_t)n * 8))) return rc;
    if ((rc = xfer_h2d(ctx, f.desc, desc, (size_t)n * 32))) return rc;
    if (n > 0) {
        VO_HIP(ctx, hipMemsetAsync(f.kp_size, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_angle, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_resp, 0, (size_t)n * 4, ctx->stream));
        VO_HIP(ctx, hipMemsetAsync(f.kp_oct, 0, (size_t)n * 4, ctx->stream));
    }
    if ((rc = xfer_flush(ctx))) return rc;
    if (++ctx->sweep_gen_next <= 0) ctx->sweep_gen_next = 1;     // a generation of its own, as every SGBM run gets: no sweep ever wrote it into the slot's word
    f.disp_gen = ctx->sweep_gen_next;
    f.w = w; f.h = h;
    *f.n_kp_host = n;
    f.n_kp = n;
    f.has_disp = true; f.has_kp = true;
    return VO_OK;
}

// ... and a dense slot that HOLDS ITS PAIR too: vo_test_plant_dense, then the w x h grey image `left` as the slot's rectified left
// and right image -- the slot stands as an upload, a synchronous vo_sgbm_compute and an ORB extraction leave it.  The seam through
// which the tests drive the Lucas-Kanade PnP step (vo_klt_pnp_pair), which tracks in the slot's image and looks its keypoints up in
// the slot's disparity.
extern "C" int vo_test_plant_dense_pair(vo_ctx* ctx, int slot, int w, int h, const uint8_t* left, const int16_t* disp16, int n, const float* xy,
                                        const uint8_t* desc)
{
    if (ctx && !left) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_dense_pair: null pointer");
    if (int rc = vo_test_plant_dense(ctx, slot, w, h, disp16, n, xy, desc)) return rc;
    FrameSlot& f = ctx->slots[slot];
    int rc;
    if ((rc = xfer_h2d(ctx, f.left, left, (size_t)w * h)) || (rc = xfer_h2d(ctx, f.right, left, (size_t)w * h)) || (rc = xfer_flush(ctx))) return rc;
    f.has_pair = true;
    return VO_OK;
}

// ... and n landmarks written straight into a map (vo_map_create), which then stands as n insertions would have left it -- with
// any float32 bits as positions (NaN, inf: what no update ever inserts) and chosen obs / last.  The last view is void; the largest
// `last` counts as a serial used.  xyz (n, 3) float32, desc / rdesc (n, 32), octave / obs / last (n) int32, last >= 0, obs >= 1.
extern "C" int vo_test_plant_map(vo_ctx* ctx, int map, int n, const float* xyz, const uint8_t* desc, const uint8_t* rdesc, const int32_t* octave,
                                 const int32_t* obs, const int32_t* last)
{
    if (!ctx || map < 0 || map >= VO_NUM_MAPS || !ctx->maps[map].used || n < 0) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_map: bad argument");
    LandmarkMap& m = ctx->maps[map];
    if (n > m.capacity) return vo_fail(ctx, VO_E_CAP, "vo_test_plant_map: %d landmarks exceed capacity %d", n, m.capacity);
    if (n > 0 && (!xyz || !desc || !rdesc || !octave || !obs || !last)) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_map: null pointer");
    int top = -1;
    for (int i = 0; i < n; i++) {
        if (last[i] < 0 || obs[i] < 1) return vo_fail(ctx, VO_E_ARG, "vo_test_plant_map: need last >= 0 and obs >= 1");
        if (last[i] > top) top = last[i];
    }
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const MapSet& s = m.set[m.cur];
    int rc;
    if ((rc = xfer_h2d(ctx, s.xyz, xyz, (size_t)n * 12)) || (rc = xfer_h2d(ctx, s.desc, desc, (size_t)n * 32)) ||
        (rc = xfer_h2d(ctx, s.rdesc, rdesc, (size_t)n * 32)) || (rc = xfer_h2d(ctx, s.oct, octave, (size_t)n * 4)) ||
        (rc = xfer_h2d(ctx, s.obs, obs, (size_t)n * 4)) || (rc = xfer_h2d(ctx, s.last, last, (size_t)n * 4)) || (rc = xfer_flush(ctx)))
        return rc;
    m.n = n; m.view_n = 0; m.max_serial = top;
    return VO_OK;
}

// ... and a look at what vo_track_map left BEHIND the keypoints the view slot admits to: the first n rows of the slot's keypoint
// arrays (the padding of the padded view lies in [visible, map size)) and of the map's view_src, whatever the slot's count says.
// Any output may be NULL.
extern "C" int vo_test_peek_view(vo_ctx* ctx, int map, int slot, int n, float* xy, float* xyz, int32_t* octave, uint8_t* desc, uint8_t* rdesc,
                                 int32_t* view_src)
{
    if (!ctx || map < 0 || map >= VO_NUM_MAPS || !ctx->maps[map].used || slot < 0 || slot >= VO_NUM_SLOTS || n < 0 || n > ctx->kp_cap)
        return vo_fail(ctx, VO_E_ARG, "vo_test_peek_view: bad argument");
    if (n == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const FrameSlot& f = ctx->slots[slot];
    int rc = VO_OK;
    if (xy) rc = xfer_d2h(ctx, xy, f.kp_xy, (size_t)n * 8);
    if (xyz && !rc) rc = xfer_d2h(ctx, xyz, f.kp_xyz, (size_t)n * 12);
    if (octave && !rc) rc = xfer_d2h(ctx, octave, f.kp_oct, (size_t)n * 4);
    if (desc && !rc) rc = xfer_d2h(ctx, desc, f.desc, (size_t)n * 32);
    if (rdesc && !rc) rc = xfer_d2h(ctx, rdesc, f.kp_rdesc, (size_t)n * 32);
    if (view_src && !rc) rc = xfer_d2h(ctx, view_src, ctx->maps[map].view_src, (size_t)n * 4);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// ... and a look at one level of the Lucas-Kanade pyramids as the last vo_klt_track_host left them: the w_l x h_l bytes at level
// `level` of image `which` (0 = A, 1 = B) of the workspace, copied on the context's stream.  The caller states the level's size (the
// workspace keeps none): it must fit what the workspace lays out for that level, ((max_w + 1) / 2 ...) x ((max_h + 1) / 2 ...).
// Level 0 is the uploaded image itself.  VO_E_STATE while the workspace was never prepared.
extern "C" int vo_test_klt_level(vo_ctx* ctx, int which, int level, int w_l, int h_l, uint8_t* out)
{
    if (!ctx || which < 0 || which > 1 || level < 0 || level >= VO_KLT_MAX_LEVELS || w_l <= 0 || h_l <= 0 || !out)
        return vo_fail(ctx, VO_E_ARG, "vo_test_klt_level: bad argument");
    int mw = ctx->max_w, mh = ctx->max_h;
    for (int l = 0; l < level; l++) { mw = (mw + 1) / 2; mh = (mh + 1) / 2; }
    if (w_l > mw || h_l > mh) return vo_fail(ctx, VO_E_CAP, "vo_test_klt_level: %dx%d exceeds level %d of the workspace (%dx%d)", w_l, h_l, level, mw, mh);
    const KltWs& k = ctx->main_mw.klt;
    if (!k.ready) return vo_fail(ctx, VO_E_STATE, "vo_test_klt_level: no Lucas-Kanade call has prepared the workspace");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = xfer_d2h(ctx, out, k.pyr[which] + k.off[level], (size_t)w_l * h_l)) { (void)xfer_flush(ctx); return rc; }
    return xfer_flush(ctx);
}
#endif
