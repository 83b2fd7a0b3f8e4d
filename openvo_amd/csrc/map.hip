// Landmark map on the device: frame-to-map tracking for the sparse stereo odometer (include/vo355.h, vo_map_*).
// NOT part of the reference (every pose of openVO is the pose of one pair of frames, stereo_odometer.py:115-160): defined by this
// build, restated in numpy by tests/map_ref.py.  Two kernels, each ONE workgroup of 1024 threads that loops over the arrays: the
// sizes (at most kp_cap entries) make them latency-bound single blocks like the pose chain's prep kernels, ordered compaction is a
// ballot prefix inside the workgroup (as k_ratio_compact / k_pnp_prep), and nothing is handed between workgroups -- no ticket, no
// fence.  Every index a kernel reads through has been range-checked on the host: a refused call, never a wrong result.
// vo_track_map chains the two around the PnP step with ONE synchronisation (restated by tests/map_fused_ref.py): k_map_view_pad (the
// view, padded to the map's size so that the launches behind it need not know the visible count), k_map_decide (one wave: the
// odometer's decisions, gates, the composed pose and its inverse) and k_map_update_dev (the update fed from device memory, which
// makes the range checks itself: nothing stands in front of it).  The arithmetic of view and update is shared code.
#include <math.h>
#include "vo_internal.h"

#define MAP_THREADS 1024
#define MAP_WAVES (MAP_THREADS / 64)

struct MapPose { double r[12]; };      // row-major 3x4: R | t

// T(Rt, p) of the header: float32 point -> float32 point through float64, three-term sums left to right (the build has no FMA
// contraction)
__device__ __forceinline__ void map_transform(const MapPose& P, float x, float y, float z, float& o0, float& o1, float& o2)
{
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    o0 = (float)(((P.r[0] * dx + P.r[1] * dy) + P.r[2] * dz) + P.r[3]);
    o1 = (float)(((P.r[4] * dx + P.r[5] * dy) + P.r[6] * dz) + P.r[7]);
    o2 = (float)(((P.r[8] * dx + P.r[9] * dy) + P.r[10] * dz) + P.r[11]);
}

__device__ __forceinline__ bool finite3(float a, float b, float c)
{
    return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}

// One trip of an ordered compaction: every thread of the workgroup calls it (uniform control flow) with its own flag -> the rank of
// this thread's entry among the kept entries of the trip, *total = how many the trip keeps.  s_cnt: MAP_WAVES words of LDS.
__device__ __forceinline__ int map_block_rank(bool keep, int* s_cnt, int* total)
{
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; w++) {
        const int c = s_cnt[w];
        tot += c;
        before += w < wave ? c : 0;
    }
    __syncthreads();                   // (the words are free for the next trip)
    *total = tot;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// a 32-byte descriptor as two 16-byte vector moves
__device__ __forceinline__ void map_copy_desc(uint8_t* __restrict__ dst, size_t di, const uint8_t* __restrict__ src, size_t si)
{
    const uint4 a = ((const uint4*)src)[2 * si], b = ((const uint4*)src)[2 * si + 1];
    ((uint4*)dst)[2 * di] = a;
    ((uint4*)dst)[2 * di + 1] = b;
}

struct MapViewOut {
    float *kp_xy, *kp_xyz, *kp_size, *kp_angle, *kp_resp, *kp_disp;
    int32_t* kp_oct;
    uint8_t *desc, *rdesc;
};

// The rows of a view (vo_map_view, step a of vo_track_map): landmark l = trip * 1024 + thread; the visible ones leave in map order.
// Every thread of the workgroup calls it -> the visible count.  first (may be NULL; LDS): {landmark, u bits, v bits} of row 0
__device__ __forceinline__ int map_view_rows(const MapSet& m, int n, const MapPose& P, double fx, double fy, double cx, double cy, float z_min,
                                             float ox, float oy, float umax, float vmax, const MapViewOut& o, int32_t* __restrict__ view_src,
                                             int* s_cnt, int* first)
{
    int out = 0;
    for (int b0 = 0; b0 < n; b0 += MAP_THREADS) {
        const int l = b0 + (int)threadIdx.x;
        bool vis = false;
        float X0 = 0.f, X1 = 0.f, X2 = 0.f, u = 0.f, v = 0.f;
        if (l < n) {
            map_transform(P, m.xyz[3 * (size_t)l], m.xyz[3 * (size_t)l + 1], m.xyz[3 * (size_t)l + 2], X0, X1, X2);
            u = (float)(fx * ((double)X0 / (double)X2) + cx) - ox;
            v = (float)(fy * ((double)X1 / (double)X2) + cy) - oy;
            vis = finite3(X0, X1, X2) && X2 >= z_min && u >= 0.f && u <= umax && v >= 0.f && v <= vmax;
        }
        int tot;
        const int r = map_block_rank(vis, s_cnt, &tot);
        if (vis) {
            const size_t k = (size_t)(out + r);
            o.kp_xy[2 * k] = u; o.kp_xy[2 * k + 1] = v;
            o.kp_xyz[3 * k] = X0; o.kp_xyz[3 * k + 1] = X1; o.kp_xyz[3 * k + 2] = X2;
            o.kp_size[k] = 0.f; o.kp_angle[k] = 0.f; o.kp_resp[k] = 0.f;
            o.kp_disp[k] = __int_as_float(0x7fc00000);
            o.kp_oct[k] = m.oct[l];
            map_copy_desc(o.desc, k, m.desc, (size_t)l);
            map_copy_desc(o.rdesc, k, m.rdesc, (size_t)l);
            view_src[k] = l;
            if (first && k == 0) { first[0] = l; first[1] = __float_as_int(u); first[2] = __float_as_int(v); }
        }
        out += tot;
    }
    return out;
}

// vo_map_view.  counts: pinned host memory {map size, visible}
__global__ __launch_bounds__(MAP_THREADS) void k_map_view(MapSet m, int n, MapPose P, double fx, double fy, double cx, double cy, float z_min,
                                                          float ox, float oy, float umax, float vmax, MapViewOut o, int32_t* __restrict__ view_src,
                                                          int32_t* __restrict__ counts)
{
    __shared__ int s_cnt[MAP_WAVES];
    const int out = map_view_rows(m, n, P, fx, fy, cx, cy, z_min, ox, oy, umax, vmax, o, view_src, s_cnt, nullptr);
    if (threadIdx.x == 0) { counts[0] = n; counts[1] = out; }
}

// Step a of vo_track_map: the view, then rows [vis, n) as padding -- clones of row 0 (position, octave, both descriptors; read from
// the MAP through the landmark row 0 came from, never from the rows this launch has just written) with a NaN 3-D point, zeros when
// nothing is visible -- so that the launches behind can be shaped for n.  vis_dev: a device word; vis_host: pinned host memory.
__global__ __launch_bounds__(MAP_THREADS) void k_map_view_pad(MapSet m, int n, MapPose P, double fx, double fy, double cx, double cy, float z_min,
                                                              float ox, float oy, float umax, float vmax, MapViewOut o,
                                                              int32_t* __restrict__ view_src, int32_t* __restrict__ vis_dev,
                                                              int32_t* __restrict__ vis_host)
{
    __shared__ int s_cnt[MAP_WAVES];
    __shared__ int s_first[3];
    const int vis = map_view_rows(m, n, P, fx, fy, cx, cy, z_min, ox, oy, umax, vmax, o, view_src, s_cnt, s_first);
    __syncthreads();                   // (s_first, written by the thread that held row 0)
    if (threadIdx.x == 0) { *vis_dev = vis; *vis_host = vis; }
    const float nan = __int_as_float(0x7fc00000);
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0, r0 = d0, r1 = d0;
    float u = 0.f, v = 0.f;
    int oct = 0;
    if (vis > 0) {
        const size_t l = (size_t)s_first[0];
        u = __int_as_float(s_first[1]); v = __int_as_float(s_first[2]);
        oct = m.oct[l];
        d0 = ((const uint4*)m.desc)[2 * l]; d1 = ((const uint4*)m.desc)[2 * l + 1];
        r0 = ((const uint4*)m.rdesc)[2 * l]; r1 = ((const uint4*)m.rdesc)[2 * l + 1];
    }
    for (int k = vis + (int)threadIdx.x; k < n; k += MAP_THREADS) {
        o.kp_xy[2 * (size_t)k] = u; o.kp_xy[2 * (size_t)k + 1] = v;
        o.kp_xyz[3 * (size_t)k] = nan; o.kp_xyz[3 * (size_t)k + 1] = nan; o.kp_xyz[3 * (size_t)k + 2] = nan;
        o.kp_size[k] = 0.f; o.kp_angle[k] = 0.f; o.kp_resp[k] = 0.f;
        o.kp_disp[k] = nan;
        o.kp_oct[k] = oct;
        ((uint4*)o.desc)[2 * (size_t)k] = d0; ((uint4*)o.desc)[2 * (size_t)k + 1] = d1;
        ((uint4*)o.rdesc)[2 * (size_t)k] = r0; ((uint4*)o.rdesc)[2 * (size_t)k + 1] = r1;
    }
}

struct MapFrame {                      // the keypoints of the frame being folded in
    const float* xyz;
    const uint8_t *desc, *rdesc;
    const int32_t* oct;
    int n;
};

// The fusion of vo_map_update (and of vo_track_map's last step): observations into set `a` in place (no landmark is named twice: a
// view lists a landmark once, and a q is named once among the inliers), then survivors and insertions into set `d`.  Every thread
// of the workgroup calls it.  counts: the six of the header.
__device__ __forceinline__ void map_fuse(const MapSet& a, const MapSet& d, int n_map, int capacity, const int32_t* __restrict__ view_src,
                                         const int32_t* __restrict__ q_idx, const int32_t* __restrict__ t_idx, const uint8_t* __restrict__ mask,
                                         int n, const MapFrame& f, const MapPose& P, int serial, int max_age, int max_obs,
                                         uint8_t* __restrict__ claimed, int32_t* __restrict__ counts)
{
    __shared__ int s_cnt[MAP_WAVES];
    __shared__ int s_obs, s_skip;
    if (threadIdx.x == 0) { s_obs = 0; s_skip = 0; }
    for (int t = threadIdx.x; t < f.n; t += MAP_THREADS) claimed[t] = 0;
    __syncthreads();
    // 1. observations
    for (int c = threadIdx.x; c < n; c += MAP_THREADS) {
        if (!mask[c]) continue;
        const int l = view_src[q_idx[c]], t = t_idx[c];
        float X0, X1, X2;
        map_transform(P, f.xyz[3 * (size_t)t], f.xyz[3 * (size_t)t + 1], f.xyz[3 * (size_t)t + 2], X0, X1, X2);
        if (!finite3(X0, X1, X2)) { atomicAdd(&s_skip, 1); continue; }
        const int ob = a.obs[l];
        const double w = (double)((ob < max_obs ? ob : max_obs) + 1);
        float* p = a.xyz + 3 * (size_t)l;
        p[0] = (float)((double)p[0] + ((double)X0 - (double)p[0]) / w);
        p[1] = (float)((double)p[1] + ((double)X1 - (double)p[1]) / w);
        p[2] = (float)((double)p[2] + ((double)X2 - (double)p[2]) / w);
        a.obs[l] = ob + 1;
        a.last[l] = serial;
        a.oct[l] = f.oct[t];
        map_copy_desc(a.desc, (size_t)l, f.desc, (size_t)t);
        map_copy_desc(a.rdesc, (size_t)l, f.rdesc, (size_t)t);
        claimed[t] = 1;                // (several landmarks may claim one keypoint: the same byte, the same value)
        atomicAdd(&s_obs, 1);
    }
    __syncthreads();
    // 2. survivors, in their order
    int size = 0;
    for (int b0 = 0; b0 < n_map; b0 += MAP_THREADS) {
        const int l = b0 + (int)threadIdx.x;
        const bool keep = l < n_map && serial - a.last[l] <= max_age;
        int tot;
        const int r = map_block_rank(keep, s_cnt, &tot);
        if (keep) {
            const size_t k = (size_t)(size + r);
            d.xyz[3 * k] = a.xyz[3 * (size_t)l]; d.xyz[3 * k + 1] = a.xyz[3 * (size_t)l + 1]; d.xyz[3 * k + 2] = a.xyz[3 * (size_t)l + 2];
            d.oct[k] = a.oct[l]; d.obs[k] = a.obs[l]; d.last[k] = a.last[l];
            map_copy_desc(d.desc, k, a.desc, (size_t)l);
            map_copy_desc(d.rdesc, k, a.rdesc, (size_t)l);
        }
        size += tot;
    }
    const int survivors = size;
    // 3. insertions, in keypoint order, while there is room
    int wanted = 0;
    for (int b0 = 0; b0 < f.n; b0 += MAP_THREADS) {
        const int t = b0 + (int)threadIdx.x;
        bool want = false;
        float X0 = 0.f, X1 = 0.f, X2 = 0.f;
        if (t < f.n && !claimed[t]) {
            map_transform(P, f.xyz[3 * (size_t)t], f.xyz[3 * (size_t)t + 1], f.xyz[3 * (size_t)t + 2], X0, X1, X2);
            want = finite3(X0, X1, X2);
        }
        int tot;
        const int r = map_block_rank(want, s_cnt, &tot);
        if (want && survivors + wanted + r < capacity) {
            const size_t k = (size_t)(survivors + wanted + r);
            d.xyz[3 * k] = X0; d.xyz[3 * k + 1] = X1; d.xyz[3 * k + 2] = X2;
            d.oct[k] = f.oct[t]; d.obs[k] = 1; d.last[k] = serial;
            map_copy_desc(d.desc, k, f.desc, (size_t)t);
            map_copy_desc(d.rdesc, k, f.rdesc, (size_t)t);
        }
        wanted += tot;
    }
    if (threadIdx.x == 0) {
        const int room = capacity - survivors, inserted = wanted < room ? wanted : room;
        counts[0] = s_obs; counts[1] = s_skip; counts[2] = n_map - survivors;
        counts[3] = inserted; counts[4] = wanted - inserted; counts[5] = survivors + inserted;
    }
}

// vo_map_update.  Every index the kernel reads through has been range-checked on the host.  counts: pinned host memory
__global__ __launch_bounds__(MAP_THREADS) void k_map_update(MapSet a, MapSet d, int n_map, int capacity, const int32_t* __restrict__ view_src,
                                                            const int32_t* __restrict__ q_idx, const int32_t* __restrict__ t_idx,
                                                            const uint8_t* __restrict__ mask, int n, MapFrame f, MapPose P, int serial, int max_age,
                                                            int max_obs, uint8_t* __restrict__ claimed, int32_t* __restrict__ counts)
{
    map_fuse(a, d, n_map, capacity, view_src, q_idx, t_idx, mask, n, f, P, serial, max_age, max_obs, claimed, counts);
}

// What the kernels of vo_track_map hand each other in device memory (LandmarkMap::d_track), and the part of the record the map's own
// kernels write into pinned host memory (the PnP step's record lies in front of it)
struct MapTrackDev {
    int32_t vis, decision;
    PnpRec pnp;
    double cw[12], wc[12];             // c_T_w of the new frame and its rigid inverse (decision 0)
};
struct MapTrackTail {
    int32_t vis, decision, update_flags, pad;
    int32_t counts6[6], pad2[2];
    double cw[12], wc[12];
};

// Step c / d of vo_track_map in one wave (one lane works: two dozen scalar decisions): the decisions of the odometer's PnP step and
// its motion gates in their order, then the composed pose and its rigid inverse.  The build contracts no multiply-add.
// poison (the test-only build's VO_FAULT_MAP_NAN, 0 everywhere else): entry 5 of the pose reads NaN
__global__ __launch_bounds__(64) void k_map_decide(MapTrackDev* __restrict__ td, MapPose Pp, int min_matches, double max_dist, double max_rot,
                                                   MapTrackTail* __restrict__ tail, int poison)
{
    if (threadIdx.x != 0) return;
    const PnpRec& r = td->pnp;
    const int vis = td->vis;
    double T[12];
    for (int k = 0; k < 12; k++) T[k] = r.rstatus == 0 ? r.Rtr[k] : r.Rt[k];
    if (poison) T[5] = __longlong_as_double(0x7ff8000000000000LL);
    int dec = 0;
    if (vis < (min_matches > 2 ? min_matches : 2) || vis > VO_MAP_TRACK_MAX) dec = 1;
    else if (r.M < min_matches) dec = 2;
    else if (r.flags & 2) dec = 8;
    else if (r.n < (min_matches > 4 ? min_matches : 4)) dec = 3;
    else if (r.best_count < min_matches) dec = 4;
    else {
        bool nan = false;
        for (int k = 0; k < 12; k++) nan = nan || T[k] != T[k];
        if (nan) dec = 5;
        else {
            const double dist = sqrt((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]);
            const double a = T[9] - T[6], b = T[2] - T[8], c = T[4] - T[1];
            const double s = sqrt((a * a + b * b) + c * c) / 2.0, co = (((T[0] + T[5]) + T[10]) - 1.0) / 2.0;
            const double angle = atan2(s, co);
            if (dist > max_dist) dec = 6;
            if (angle > max_rot) dec = 7;
        }
    }
    double cw[12], wc[12];
    for (int k = 0; k < 12; k++) cw[k] = wc[k] = 0.0;
    if (dec == 0) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++)
                cw[4 * i + j] = ((T[4 * i] * Pp.r[j] + T[4 * i + 1] * Pp.r[4 + j]) + T[4 * i + 2] * Pp.r[8 + j]) + T[4 * i + 3] * (j == 3 ? 1.0 : 0.0);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) wc[4 * i + j] = cw[4 * j + i];
            wc[4 * i + 3] = -((cw[i] * cw[3] + cw[4 + i] * cw[7]) + cw[8 + i] * cw[11]);
        }
    }
    td->decision = dec;
    tail->decision = dec;
    for (int k = 0; k < 12; k++) { td->cw[k] = cw[k]; td->wc[k] = wc[k]; tail->cw[k] = cw[k]; tail->wc[k] = wc[k]; }
}

// Step d of vo_track_map: vo_map_update fed from device memory -- the correspondences k_pnp_prep compacted (hdr[1] of them, at most
// n_cap), the mask k_pnp_finish left, the pose and the decision of k_map_decide.  No host check stands in front of it, so it checks
// every index it would read through FIRST (unsigned compares: a negative index fails too): one violation and nothing is applied.
__global__ __launch_bounds__(MAP_THREADS) void k_map_update_dev(MapSet a, MapSet d, int n_map, int capacity, const int32_t* __restrict__ view_src,
                                                                const int32_t* __restrict__ q_idx, const int32_t* __restrict__ t_idx,
                                                                const uint8_t* __restrict__ mask, const int32_t* __restrict__ hdr, int n_cap,
                                                                MapFrame f, const MapTrackDev* __restrict__ td, int serial, int max_age, int max_obs,
                                                                uint8_t* __restrict__ claimed, MapTrackTail* __restrict__ tail)
{
    const bool accept = td->decision == 0;         // (uniform: every thread reads the same words)
    int n = hdr[1];
    n = n < 0 ? 0 : (n > n_cap ? n_cap : n);
    const unsigned vis = (unsigned)td->vis;
    int bad = 0;
    if (accept)
        for (int c = threadIdx.x; c < n; c += MAP_THREADS)
            if (mask[c] && ((unsigned)q_idx[c] >= vis || (unsigned)t_idx[c] >= (unsigned)f.n)) bad = 1;
    bad = __syncthreads_or(bad);
    if (!accept || bad) {
        if (threadIdx.x == 0) {
            for (int i = 0; i < 6; i++) tail->counts6[i] = -1;
            tail->update_flags = bad ? 1 : 0;
        }
        return;
    }
    if (threadIdx.x == 0) tail->update_flags = 0;
    MapPose P;
    for (int k = 0; k < 12; k++) P.r[k] = td->wc[k];
    map_fuse(a, d, n_map, capacity, view_src, q_idx, t_idx, mask, n, f, P, serial, max_age, max_obs, claimed, tail->counts6);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
void map_free(LandmarkMap& m)
{
    for (MapSet& s : m.set) {
        void* ps[] = { s.xyz, s.desc, s.rdesc, s.oct, s.obs, s.last };
        for (void* p : ps) if (p) (void)hipFree(p);
    }
    void* ps[] = { m.view_src, m.d_q, m.d_t, m.claimed, m.d_mask, m.d_track };
    for (void* p : ps) if (p) (void)hipFree(p);
    m = LandmarkMap();
}

static int map_get(vo_ctx* ctx, int map, const char* who, LandmarkMap** out)
{
    if (!ctx) return VO_E_ARG;
    if (map < 0 || map >= VO_NUM_MAPS || !ctx->maps[map].used) return vo_fail(ctx, VO_E_ARG, "%s: %d is not a map of this context", who, map);
    *out = &ctx->maps[map];
    return VO_OK;
}

static bool all_finite(const double* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int vo_map_create(vo_ctx* ctx, int capacity, int* map_out)
{
    if (!ctx) return VO_E_ARG;
    if (!map_out) return vo_fail(ctx, VO_E_ARG, "vo_map_create: bad argument");
    *map_out = -1;
    if (capacity < 16 || capacity > ctx->kp_cap)
        return vo_fail(ctx, VO_E_ARG, "vo_map_create: need 16 <= capacity <= %d (a view must fit a frame slot), not %d", ctx->kp_cap, capacity);
    int k = 0;
    while (k < VO_NUM_MAPS && ctx->maps[k].used) k++;
    if (k == VO_NUM_MAPS) return vo_fail(ctx, VO_E_CAP, "vo_map_create: a context holds at most %d maps", VO_NUM_MAPS);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    LandmarkMap& m = ctx->maps[k];
    const size_t cap = (size_t)capacity, kc = (size_t)ctx->kp_cap;
    hipError_t e = hipSuccess;
    auto take = [&e](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes + 256); };
    for (MapSet& s : m.set) {
        take((void**)&s.xyz, cap * 12); take((void**)&s.desc, cap * 32); take((void**)&s.rdesc, cap * 32);
        take((void**)&s.oct, cap * 4); take((void**)&s.obs, cap * 4); take((void**)&s.last, cap * 4);
    }
    take((void**)&m.view_src, kc * 4); take((void**)&m.d_q, kc * 4); take((void**)&m.d_t, kc * 4);
    take((void**)&m.claimed, kc); take((void**)&m.d_track, sizeof(MapTrackDev));
    take((void**)&m.d_mask, kc);
    if (e != hipSuccess) {
        map_free(m);
        return vo_fail(ctx, VO_E_HIP, "vo_map_create: hipMalloc failed: %s", hipGetErrorString(e));
    }
    m.seen.assign(kc, 0);
    m.used = true;
    m.capacity = capacity;
    *map_out = k;
    return VO_OK;
}

extern "C" int vo_map_destroy(vo_ctx* ctx, int map)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_map_destroy", &m)) return rc;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    map_free(*m);
    return VO_OK;
}

extern "C" int vo_map_reset(vo_ctx* ctx, int map)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_map_reset", &m)) return rc;
    m->n = 0; m->view_n = 0; m->max_serial = -1;
    return VO_OK;
}

extern "C" int vo_map_view(vo_ctx* ctx, int map, const double* Rt12_cw, const double* K4v, float z_min, int ref_slot, int view_slot,
                           int32_t* counts2)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_map_view", &m)) return rc;
    if (!Rt12_cw || !K4v || !counts2 || ref_slot < 0 || ref_slot >= VO_NUM_SLOTS || view_slot < 0 || view_slot >= VO_NUM_SLOTS)
        return vo_fail(ctx, VO_E_ARG, "vo_map_view: bad argument");
    if (view_slot == ref_slot) return vo_fail(ctx, VO_E_ARG, "vo_map_view: the view cannot go into the slot it will be matched against");
    if (!all_finite(Rt12_cw, 12) || !all_finite(K4v, 4) || !(K4v[0] > 0.0) || !(K4v[1] > 0.0) || !std::isfinite(z_min) || z_min < 0.f)
        return vo_fail(ctx, VO_E_ARG, "vo_map_view: need a finite pose, finite K4 with positive focal lengths and a finite z_min >= 0");
    FrameSlot& ref = ctx->slots[ref_slot];
    FrameSlot& f = ctx->slots[view_slot];
    if (!ref.has_pair) return vo_fail(ctx, VO_E_STATE, "vo_map_view: slot %d holds no image (its crop places the view)", ref_slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    // the crop of orb_slots_enqueue for ref_slot's image
    int x0 = 0, y0 = 0, x1 = ref.w, y1 = ref.h;
    if (ctx->has_roi) { x0 = ctx->roi[0]; y0 = ctx->roi[1]; x1 = ctx->roi[2] < ref.w ? ctx->roi[2] : ref.w; y1 = ctx->roi[3] < ref.h ? ctx->roi[3] : ref.h; }
    const int cw = x1 - x0, ch = y1 - y0;
    int rc;
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;     // (steps begun ahead may still read the slot)
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false; f.sp_pending = false; f.sp_ahead = false;
    f.mono_serial = 0;
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;
    f.sp_req.nfeatures = -1;                 // no request ever equals it
    m->view_n = 0;
    int32_t* counts = (int32_t*)xfer_stage(ctx, 64);
    if (!counts) {
        if ((rc = xfer_flush(ctx))) return rc;
        if (!(counts = (int32_t*)xfer_stage(ctx, 64))) return vo_fail(ctx, VO_E_CAP, "vo_map_view: the transfer arena is full");
    }
    counts[0] = m->n; counts[1] = 0;
    if (m->n > 0) {
        StageTimer t(ctx, VO_T_MATCH);
        MapPose P;
        memcpy(P.r, Rt12_cw, sizeof(P.r));
        const MapViewOut o = { f.kp_xy, f.kp_xyz, f.kp_size, f.kp_angle, f.kp_resp, f.kp_disp, f.kp_oct, f.desc, f.kp_rdesc };
        hipLaunchKernelGGL(k_map_view, dim3(1), dim3(MAP_THREADS), 0, ctx->stream, m->set[m->cur], m->n, P, K4v[0], K4v[1], K4v[2], K4v[3], z_min,
                           (float)x0, (float)y0, (float)(cw - 1), (float)(ch - 1), o, m->view_src, counts);
        VO_CHECK_LAUNCH(ctx);
    }
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    const int vis = counts[1];
    if (vis < 0 || vis > m->n) return vo_fail(ctx, VO_E_HIP, "vo_map_view: the kernel reported %d visible of %d landmarks", vis, m->n);
    counts2[0] = m->n; counts2[1] = vis;
    f.sp_rec[0] = f.sp_rec[1] = f.sp_rec[2] = f.sp_rec[3] = vis;
    *f.n_kp_host = vis;
    f.n_kp = vis;
    f.has_kp = true; f.kp_depth = true;
    m->view_n = vis;
    return VO_OK;
}

extern "C" int vo_map_update(vo_ctx* ctx, int map, int slot_new, const double* Rt12_wc, int serial, int max_age, int max_obs,
                             const int32_t* q_idx, const int32_t* t_idx, const uint8_t* mask, int n, int32_t* counts6)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_map_update", &m)) return rc;
    if (!Rt12_wc || !counts6 || slot_new < 0 || slot_new >= VO_NUM_SLOTS || n < 0 || n > ctx->kp_cap || (n > 0 && (!q_idx || !t_idx || !mask)))
        return vo_fail(ctx, VO_E_ARG, "vo_map_update: bad argument");
    if (max_age < 0 || max_obs < 1 || max_obs > 65535) return vo_fail(ctx, VO_E_ARG, "vo_map_update: need max_age >= 0 and 1 <= max_obs <= 65535");
    if (serial < 0 || serial < m->max_serial)
        return vo_fail(ctx, VO_E_ARG, "vo_map_update: serial %d is negative or below %d, used before", serial, m->max_serial);
    if (!all_finite(Rt12_wc, 12)) return vo_fail(ctx, VO_E_ARG, "vo_map_update: the pose is not finite");
    FrameSlot& f = ctx->slots[slot_new];
    if (!slot_sparse(f)) return vo_fail(ctx, VO_E_STATE, "vo_map_update: slot %d: the keypoints carry no depth (vo_sparse_stereo)", slot_new);
    for (int c = 0; c < n; c++) {
        if (q_idx[c] < 0 || q_idx[c] >= m->view_n)
            return vo_fail(ctx, VO_E_ARG, "vo_map_update: q[%d] = %d is outside the last view (%d keypoints)", c, q_idx[c], m->view_n);
        if (t_idx[c] < 0 || t_idx[c] >= f.n_kp)
            return vo_fail(ctx, VO_E_ARG, "vo_map_update: t[%d] = %d is outside slot %d (%d keypoints)", c, t_idx[c], slot_new, f.n_kp);
    }
    {
        int dup = -1;
        for (int c = 0; c < n && dup < 0; c++)
            if (mask[c]) { if (m->seen[q_idx[c]]) dup = c; else m->seen[q_idx[c]] = 1; }
        for (int c = 0; c < n; c++) m->seen[q_idx[c]] = 0;
        if (dup >= 0) return vo_fail(ctx, VO_E_ARG, "vo_map_update: view keypoint %d is named twice among the inliers (entry %d)", q_idx[dup], dup);
    }
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = slot_wait(ctx, f))) return rc;
    if ((rc = xfer_h2d(ctx, m->d_q, q_idx, (size_t)n * 4)) || (rc = xfer_h2d(ctx, m->d_t, t_idx, (size_t)n * 4)) ||
        (rc = xfer_h2d(ctx, m->d_mask, mask, (size_t)n)))
        return rc;
    int32_t* counts = (int32_t*)xfer_stage(ctx, 64);
    if (!counts) {
        if ((rc = xfer_flush(ctx))) return rc;       // (the arena was full: the copies above have landed, it is empty again)
        if (!(counts = (int32_t*)xfer_stage(ctx, 64))) return vo_fail(ctx, VO_E_CAP, "vo_map_update: the transfer arena is full");
    }
    for (int i = 0; i < 6; i++) counts[i] = -1;
    {
        StageTimer t(ctx, VO_T_POSE);
        MapPose P;
        memcpy(P.r, Rt12_wc, sizeof(P.r));
        const MapFrame fr = { f.kp_xyz, f.desc, f.kp_rdesc, f.kp_oct, f.n_kp };
        hipLaunchKernelGGL(k_map_update, dim3(1), dim3(MAP_THREADS), 0, ctx->stream, m->set[m->cur], m->set[m->cur ^ 1], m->n, m->capacity, m->view_src,
                           m->d_q, m->d_t, m->d_mask, n, fr, P, serial, max_age, max_obs, m->claimed, counts);
        VO_CHECK_LAUNCH(ctx);
    }
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    if (counts[5] < 0 || counts[5] > m->capacity) return vo_fail(ctx, VO_E_HIP, "vo_map_update: the kernel reported a size of %d", counts[5]);
    for (int i = 0; i < 6; i++) counts6[i] = counts[i];
    m->cur ^= 1;
    m->n = counts[5];
    m->view_n = 0;
    m->max_serial = serial;
    return VO_OK;
}

// view + PnP step + decisions + update as one chain on ctx->stream: see the header.  Everything is checked first; the map's host
// state changes only behind the one synchronisation, and only on decision 0.  lo_rounds > 0 (vo_track_map_lo): the PnP step runs
// its LO form -- k_map_decide reads the LO pose from the record, k_map_update_dev the set S_c from the step's mask.
static int track_map_impl(vo_ctx* ctx, int map, int slot_new, int view_slot, const double* Rt12_cw_pred, const double* K4v, float z_min,
                          double ratio, int match_flags, int iters, float thr, uint32_t seed, int refine_iters, int min_matches,
                          double max_dist, double max_rot, int serial, int max_age, int max_obs, vo_track_map_rec* rec, uint8_t* mask_out,
                          int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_track_map", &m)) return rc;
    if (!Rt12_cw_pred || !K4v || !rec || slot_new < 0 || slot_new >= VO_NUM_SLOTS || view_slot < 0 || view_slot >= VO_NUM_SLOTS)
        return vo_fail(ctx, VO_E_ARG, "vo_track_map: bad argument");
    if (view_slot == slot_new) return vo_fail(ctx, VO_E_ARG, "vo_track_map: the view cannot go into the slot it will be matched against");
    if (!all_finite(Rt12_cw_pred, 12) || !all_finite(K4v, 4) || !(K4v[0] > 0.0) || !(K4v[1] > 0.0) || !std::isfinite(z_min) || z_min < 0.f)
        return vo_fail(ctx, VO_E_ARG, "vo_track_map: need a finite pose, finite K4 with positive focal lengths and a finite z_min >= 0");
    if (min_matches < 0 || max_dist != max_dist || max_rot != max_rot)
        return vo_fail(ctx, VO_E_ARG, "vo_track_map: need min_matches >= 0 and gates that are numbers");
    if (max_age < 0 || max_obs < 1 || max_obs > 65535) return vo_fail(ctx, VO_E_ARG, "vo_track_map: need max_age >= 0 and 1 <= max_obs <= 65535");
    if (serial < 0 || serial < m->max_serial)
        return vo_fail(ctx, VO_E_ARG, "vo_track_map: serial %d is negative or below %d, used before", serial, m->max_serial);
    FrameSlot& b = ctx->slots[slot_new];
    FrameSlot& f = ctx->slots[view_slot];
    if (!b.has_pair) return vo_fail(ctx, VO_E_STATE, "vo_track_map: slot %d holds no image (its crop places the view)", slot_new);
    const int n = m->n;
    LoopGate lg;
    int rc;
    if ((rc = pnp_check(ctx, view_slot, slot_new, match_flags, K4v, iters, thr, refine_iters, "vo_track_map", &lg, n))) return rc;
    if (n > VO_MAP_TRACK_MAX) return vo_fail(ctx, VO_E_CAP, "vo_track_map: a map of %d landmarks exceeds the fused step (%d)", n, VO_MAP_TRACK_MAX);
    const bool want = mask_out || q_idx || t_idx;
    if (want && cap < n) return vo_fail(ctx, VO_E_CAP, "vo_track_map: outputs hold %d entries, the map %d landmarks", cap, n);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int x0 = 0, y0 = 0, x1 = b.w, y1 = b.h;      // the crop of orb_slots_enqueue for slot_new's image
    if (ctx->has_roi) { x0 = ctx->roi[0]; y0 = ctx->roi[1]; x1 = ctx->roi[2] < b.w ? ctx->roi[2] : b.w; y1 = ctx->roi[3] < b.h ? ctx->roi[3] : b.h; }
    const int cw = x1 - x0, ch = y1 - y0;
    if ((rc = slot_wait(ctx, b)) || (rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;
    // the record's two halves and the arrays: pinned memory the kernels write themselves
    const size_t arr_bytes = n > 0 && want ? pnp_cap(ctx->kp_cap) * 9 : 0, bytes = 512 + sizeof(MapTrackTail) + arr_bytes;
    static_assert(sizeof(PnpRec) <= 512, "the PnP record lies in front of the tail");
    uint8_t* blk = (uint8_t*)xfer_stage(ctx, bytes);
    if (!blk) {
        if ((rc = xfer_flush(ctx))) return rc;
        if (!(blk = (uint8_t*)xfer_stage(ctx, bytes))) return vo_fail(ctx, VO_E_CAP, "vo_track_map: the transfer arena cannot hold %d landmarks", n);
    }
    PnpRec* prec = (PnpRec*)blk;
    MapTrackTail* tail = (MapTrackTail*)(blk + 512);
    uint8_t* arr = arr_bytes ? blk + 512 + sizeof(MapTrackTail) : nullptr;
    memset(prec, 0, sizeof(PnpRec));
    prec->rstatus = 1;
    memset(tail, 0, sizeof(MapTrackTail));
    tail->decision = 1;                        // (an empty map: nothing is visible, nothing is launched)
    for (int i = 0; i < 6; i++) tail->counts6[i] = -1;
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false; f.sp_pending = false; f.sp_ahead = false;
    f.mono_serial = 0;
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;
    f.sp_req.nfeatures = -1;                   // no request ever equals it
    m->view_n = 0;
    if (n > 0) {
        MapTrackDev* td = (MapTrackDev*)m->d_track;
        MapPose P;
        memcpy(P.r, Rt12_cw_pred, sizeof(P.r));
        {
            StageTimer t(ctx, VO_T_MATCH);
            const MapViewOut o = { f.kp_xy, f.kp_xyz, f.kp_size, f.kp_angle, f.kp_resp, f.kp_disp, f.kp_oct, f.desc, f.kp_rdesc };
            hipLaunchKernelGGL(k_map_view_pad, dim3(1), dim3(MAP_THREADS), 0, ctx->stream, m->set[m->cur], n, P, K4v[0], K4v[1], K4v[2], K4v[3], z_min,
                               (float)x0, (float)y0, (float)(cw - 1), (float)(ch - 1), o, m->view_src, &td->vis, &tail->vis);
            VO_CHECK_LAUNCH(ctx);
        }
        // for the launches behind, the slot holds n rows (the device knows how many of them are the view)
        f.n_kp = n; f.has_kp = true; f.kp_depth = true;
        PnpChain chain;
        chain.nq_dev = &td->vis; chain.rec_dev = &td->pnp;
        rc = pnp_enqueue(ctx, f, b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, prec, arr, lg, &chain, lo_rounds);
        if (!rc) {
            {
                StageTimer t(ctx, VO_T_POSE);
                const int poison = ctx->fault_map_nan > 0 && --ctx->fault_map_nan == 0;      // (only the test-hooks build ever sets it)
                hipLaunchKernelGGL(k_map_decide, dim3(1), dim3(64), 0, ctx->stream, td, P, min_matches, max_dist, max_rot, tail, poison);
            }
            {
                StageTimer t(ctx, VO_T_POSE);
                const MapFrame fr = { b.kp_xyz, b.desc, b.kp_rdesc, b.kp_oct, b.n_kp };
                hipLaunchKernelGGL(k_map_update_dev, dim3(1), dim3(MAP_THREADS), 0, ctx->stream, m->set[m->cur], m->set[m->cur ^ 1], n, m->capacity,
                                   m->view_src, chain.d.q, chain.d.t, chain.mask, chain.d.hdr, n, fr, td, serial, max_age, max_obs, m->claimed, tail);
            }
            if (hipGetLastError() != hipSuccess) rc = vo_fail(ctx, VO_E_HIP, "vo_track_map: a launch failed");
        }
        const int rcf = xfer_flush(ctx);           // the one synchronisation (also behind a failed enqueue: the view's launch is out)
        if (rc || (rc = rcf)) { f.has_kp = false; f.kp_depth = false; f.n_kp = 0; *f.n_kp_host = 0; return rc; }
    }
    const int vis = tail->vis, dec = tail->decision;
    if (vis < 0 || vis > n) { f.has_kp = false; f.kp_depth = false; f.n_kp = 0; return vo_fail(ctx, VO_E_HIP, "vo_track_map: the kernel reported %d visible of %d landmarks", vis, n); }
    f.sp_rec[0] = f.sp_rec[1] = f.sp_rec[2] = f.sp_rec[3] = vis;
    *f.n_kp_host = vis;
    f.n_kp = vis;
    f.has_kp = true; f.kp_depth = true;
    m->view_n = vis;
    rec->decision = dec; rec->map_n = n; rec->vis = vis; rec->update_flags = tail->update_flags;
    rec->M = prec->M; rec->n = prec->n; rec->best_iter = prec->best_iter; rec->best_count = prec->best_count;
    rec->flags = prec->flags; rec->rstatus = prec->rstatus; rec->rsteps = prec->rsteps;
    rec->pad = lo_rounds > 0 ? prec->lo_rounds : 0;                  // (vo_track_map_lo: rounds completed ...
    for (int i = 0; i < 6; i++) rec->counts6[i] = tail->counts6[i];
    rec->pad2[0] = lo_rounds > 0 ? prec->lo_support : 0;             //  ... and |S_c|)
    rec->pad2[1] = 0;
    memcpy(rec->Rt, prec->Rt, sizeof(rec->Rt)); memcpy(rec->Rtr, prec->Rtr, sizeof(rec->Rtr));
    memcpy(rec->c_T_w, tail->cw, sizeof(rec->c_T_w)); memcpy(rec->w_T_c, tail->wc, sizeof(rec->w_T_c));
    if (arr) {
        const size_t pc = pnp_cap(ctx->kp_cap);
        if (mask_out) memcpy(mask_out, arr, (size_t)n);
        if (q_idx) memcpy(q_idx, arr + pc, (size_t)n * 4);
        if (t_idx) memcpy(t_idx, arr + pc * 5, (size_t)n * 4);
    }
    if (dec == 8) return vo_fail(ctx, VO_E_STATE, "vo_track_map: a match index lies outside the train set: the frame is refused");
    if (tail->update_flags) return vo_fail(ctx, VO_E_STATE, "vo_track_map: a correspondence lies outside the view or the frame: nothing was applied");
    if (dec == 0) {
        if (tail->counts6[5] < 0 || tail->counts6[5] > m->capacity) return vo_fail(ctx, VO_E_HIP, "vo_track_map: the kernel reported a size of %d", tail->counts6[5]);
        m->cur ^= 1;
        m->n = tail->counts6[5];
        m->view_n = 0;
        m->max_serial = serial;
    }
    return VO_OK;
}

extern "C" int vo_track_map(vo_ctx* ctx, int map, int slot_new, int view_slot, const double* Rt12_cw_pred, const double* K4v, float z_min,
                            double ratio, int match_flags, int iters, float thr, uint32_t seed, int refine_iters, int min_matches,
                            double max_dist, double max_rot, int serial, int max_age, int max_obs, vo_track_map_rec* rec, uint8_t* mask_out,
                            int32_t* q_idx, int32_t* t_idx, int cap)
{
    return track_map_impl(ctx, map, slot_new, view_slot, Rt12_cw_pred, K4v, z_min, ratio, match_flags, iters, thr, seed, refine_iters, min_matches,
                          max_dist, max_rot, serial, max_age, max_obs, rec, mask_out, q_idx, t_idx, cap, 0);
}

extern "C" int vo_track_map_lo(vo_ctx* ctx, int map, int slot_new, int view_slot, const double* Rt12_cw_pred, const double* K4v, float z_min,
                               double ratio, int match_flags, int iters, float thr, uint32_t seed, int refine_iters, int min_matches,
                               double max_dist, double max_rot, int serial, int max_age, int max_obs, vo_track_map_rec* rec, uint8_t* mask_out,
                               int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds)
{
    if (int rc = pnp_lo_check(ctx, lo_rounds, refine_iters, "vo_track_map_lo")) return rc;
    return track_map_impl(ctx, map, slot_new, view_slot, Rt12_cw_pred, K4v, z_min, ratio, match_flags, iters, thr, seed, refine_iters, min_matches,
                          max_dist, max_rot, serial, max_age, max_obs, rec, mask_out, q_idx, t_idx, cap, lo_rounds);
}

extern "C" int vo_map_download(vo_ctx* ctx, int map, float* xyz, uint8_t* desc, int32_t* octave, int32_t* obs, int32_t* last, int cap, int* n_out)
{
    LandmarkMap* m;
    if (int rc = map_get(ctx, map, "vo_map_download", &m)) return rc;
    const int n = m->n;
    if (n_out) *n_out = n;
    const bool any = xyz || desc || octave || obs || last;
    if (n == 0 || !any) return VO_OK;
    if (n > cap) return vo_fail(ctx, VO_E_CAP, "vo_map_download: %d landmarks exceed the output capacity %d", n, cap);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    const MapSet& s = m->set[m->cur];
    int rc = VO_OK;
    if (xyz) rc = xfer_d2h(ctx, xyz, s.xyz, (size_t)n * 12);
    if (desc && !rc) rc = xfer_d2h(ctx, desc, s.desc, (size_t)n * 32);
    if (octave && !rc) rc = xfer_d2h(ctx, octave, s.oct, (size_t)n * 4);
    if (obs && !rc) rc = xfer_d2h(ctx, obs, s.obs, (size_t)n * 4);
    if (last && !rc) rc = xfer_d2h(ctx, last, s.last, (size_t)n * 4);
    if (rc) return rc;
    return xfer_flush(ctx);
}
