// Sparse stereo depth on gfx950: per-keypoint disparity from left / right ORB, no dense disparity image.
// NOT part of the reference (openVO reads a dense SGBM disparity at its keypoints, stereo_odometer.py:50-79,117): defined by this
// build, see include/vo355.h (vo_sparse_stereo) and tests/sparse_stereo_ref.py, which restates it in numpy.
//   k_sparse_match     one wave per left keypoint: association along the epipolar row (lanes over right keypoints, wave argmin
//                      on (distance << 16 | j)), then the sub-pixel refinement by 11 x 11 SAD over 11 shifts and the 3-D point
//   k_sparse_pair      the same association and refinement, and behind it -- in the workgroup that arrives last at a ticket -- the
//                      ordered compaction (ballot prefix) of the surviving left keypoints from the scratch set into the slot: ONE
//                      launch per pair (a queue entry behind other engines' kernels costs more than the two kernels it replaces)
//   k_sparse_compact   that compaction as a launch of its own (VO_SPARSE_TWO_LAUNCHES builds only: the form k_sparse_pair is measured against)
// The kernels are templates on the association tests (vo_set_sparse_assoc): the instantiation with none is the code without them.
//   ratio    the wave tracks its TWO smallest keys (each lane a private best and second, two DPP minima) and accepts the winner
//            only when it is clearly ahead of the runner-up
//   mutual   one claim word per right keypoint: every lane lowers the word of each candidate within max_hamming to
//            (distance << 16 | i) with a vector atomic minimum; the compaction, which runs behind every other workgroup's release,
//            keeps keypoint i only when the word of its winner names i, and puts the words back to 0xFFFFFFFF
// Compiled with -ffp-contract=off like the rest of the library: the float32 / float64 arithmetic below is the definition.
#include <math.h>
#include "vo_internal.h"

#define SP_W 5     // half width of the SAD window (11 x 11)
#define SP_L 5     // shifts -L .. L around the associated right keypoint
#define SP_MUTUAL VO_SPARSE_MUTUAL
#define SP_RATIO VO_SPARSE_RATIO

struct SparseP {
    float min_disp, max_disp, row_tol;
    int max_hamming;
    float sc[VO_ORB_LEVELS];       // (float)pow((double)1.2f, o)
    double Q[16];
    float x0f, y0f;                // ROI origin (float32 add onto the keypoint position)
};

__device__ __forceinline__ unsigned sp_wave_min_u32(unsigned v)
{
#define DPP_MIN(ctrl, rmask) v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xf, false))
    DPP_MIN(0x111, 0xf); DPP_MIN(0x112, 0xf); DPP_MIN(0x114, 0xf); DPP_MIN(0x118, 0xf);
    DPP_MIN(0x142, 0xa); DPP_MIN(0x143, 0xc);
#undef DPP_MIN
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ int sp_wave_sum_i32(int v)
{
#define DPP_ADD(ctrl, rmask) v += __builtin_amdgcn_update_dpp(0, v, ctrl, rmask, 0xf, false)
    DPP_ADD(0x111, 0xf); DPP_ADD(0x112, 0xf); DPP_ADD(0x114, 0xf); DPP_ADD(0x118, 0xf);
    DPP_ADD(0x142, 0xa); DPP_ADD(0x143, 0xc);
#undef DPP_ADD
    return __builtin_amdgcn_readlane(v, 63);
}

// first index in [0, n) whose octave is >= o (the octaves are non-decreasing)
__device__ __forceinline__ int sp_lower_bound(const int32_t* __restrict__ oct, int n, int o)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (oct[mid] < o) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// nl_p / nr_p: the keypoint counts as the two extractions left them (pinned host words; clamped to cap).  sorted_r: the right
// octaves are non-decreasing (ORB's canonical order), so the candidates lie in one index range found by two binary searches.
// imgL / imgR: the two crops (cw x ch, `stride` bytes per row).  xyz may be NULL (host seam: no 3-D point).
// One wave: left keypoint i (< nl) of the keypoint sets below.  match / disp / xyz are plain pointers: k_sparse_pair reads them back
// in the same launch behind an agent-scope acquire, and bytes handed over that way must stay off the scalar path.  claim: the words
// of the mutual test (read only with SP_MUTUAL); ratio: of the ratio test (read only with SP_RATIO).
template <int FLAGS>
__device__ __forceinline__ void sparse_match_one(int i, int lane, int nr,
                                                 const float* __restrict__ xy_l, const int32_t* __restrict__ oct_l, const uint8_t* __restrict__ desc_l,
                                                 const float* __restrict__ xy_r, const int32_t* __restrict__ oct_r, const uint8_t* __restrict__ desc_r,
                                                 int sorted_r, const uint8_t* __restrict__ imgL, const uint8_t* __restrict__ imgR, int stride,
                                                 int cw, int ch, const SparseP& P, int32_t* match, float* disp, float* xyz,
                                                 float ratio, uint32_t* claim)
{
    const float nanf_ = __builtin_nanf("");
    const float xi = xy_l[2 * i], yi = xy_l[2 * i + 1];
    const int oi = oct_l[i];
    unsigned key = 0xFFFFFFFFu, key2 = 0xFFFFFFFFu;      // (a real key is below 257 << 16)
    if (nr <= 65535 && (unsigned)oi < VO_ORB_LEVELS) {
        int lo = 0, hi = nr;
        if (sorted_r) { lo = sp_lower_bound(oct_r, nr, oi - 1); hi = sp_lower_bound(oct_r, nr, oi + 2); }
        const float tol = P.row_tol * P.sc[oi];
        const uint4 a0 = ((const uint4*)desc_l)[2 * (size_t)i], a1 = ((const uint4*)desc_l)[2 * (size_t)i + 1];
        for (int j = lo + lane; j < hi; j += 64) {
            const int dd = oi - oct_r[j];
            if (dd < -1 || dd > 1) continue;
            if (!(fabsf(yi - xy_r[2 * j + 1]) <= tol)) continue;
            const float d0 = xi - xy_r[2 * j];
            if (!(d0 >= P.min_disp && d0 <= P.max_disp)) continue;
            const uint4 b0 = ((const uint4*)desc_r)[2 * (size_t)j], b1 = ((const uint4*)desc_r)[2 * (size_t)j + 1];
            const int dist = (__popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y)) + (__popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w)) +
                             (__popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y)) + (__popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w));
            const unsigned k = ((unsigned)dist << 16) | (unsigned)j;
            if (FLAGS & SP_RATIO) key2 = min(key2, max(key, k));
            key = min(key, k);
            if ((FLAGS & SP_MUTUAL) && dist <= P.max_hamming && i <= 65535)
                (void)__hip_atomic_fetch_min(claim + j, ((unsigned)dist << 16) | (unsigned)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (FLAGS & SP_RATIO) {
            // the keys are distinct (j is): exactly one lane holds the wave's smallest, and the runner-up is the smallest of its
            // second and every other lane's best
            const unsigned k1 = sp_wave_min_u32(key);
            key2 = sp_wave_min_u32(key == k1 ? key2 : key);
            key = k1;
        } else {
            key = sp_wave_min_u32(key);
        }
    }
    bool ok = key != 0xFFFFFFFFu && (int)(key >> 16) <= P.max_hamming;
    if ((FLAGS & SP_RATIO) && ok && key2 != 0xFFFFFFFFu) ok = (float)(key >> 16) < ratio * (float)(key2 >> 16);
    if (!ok) {                                                            // (wave-uniform from here on)
        if (lane == 0) { match[i] = -1; disp[i] = nanf_; }
        return;
    }
    const int j = (int)(key & 0xFFFFu);
    if (lane == 0) match[i] = j;
    // refinement at full resolution: the windows are tested in float32 before anything is converted (a coordinate may be huge)
    const float fx0 = rintf(xi), fy0 = rintf(yi), fxr = rintf(xy_r[2 * j]);
    const bool inside = fx0 - SP_W >= 0.f && fx0 + SP_W <= (float)(cw - 1) && fy0 - SP_W >= 0.f && fy0 + SP_W <= (float)(ch - 1) &&
                        fxr - (SP_W + SP_L) >= 0.f && fxr + (SP_W + SP_L) <= (float)(cw - 1);
    if (!inside) {
        if (lane == 0) disp[i] = nanf_;
        return;
    }
    const int x0 = (int)fx0, y0 = (int)fy0, xr = (int)fxr;
    int sad[2 * SP_L + 1];
#pragma unroll
    for (int s = 0; s <= 2 * SP_L; s++) sad[s] = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int p = lane + 64 * k;
        if (p < (2 * SP_W + 1) * (2 * SP_W + 1)) {
            const int dy = p / (2 * SP_W + 1) - SP_W, dx = p % (2 * SP_W + 1) - SP_W;
            const int l = imgL[(size_t)(y0 + dy) * stride + (x0 + dx)];
            const uint8_t* r = imgR + (size_t)(y0 + dy) * stride + (xr + dx - SP_L);
#pragma unroll
            for (int s = 0; s <= 2 * SP_L; s++) sad[s] += abs(l - (int)r[s]);
        }
    }
#pragma unroll
    for (int s = 0; s <= 2 * SP_L; s++) sad[s] = sp_wave_sum_i32(sad[s]);
    if (lane != 0) return;
    int sb = 0;
#pragma unroll
    for (int s = 1; s <= 2 * SP_L; s++) if (sad[s] < sad[sb]) sb = s;          // the first minimum
    float d = nanf_;
    if (sb != 0 && sb != 2 * SP_L) {
        int sm = 0, s0 = 0, sp = 0;
#pragma unroll
        for (int s = 1; s < 2 * SP_L; s++) if (s == sb) { sm = sad[s - 1]; s0 = sad[s]; sp = sad[s + 1]; }
        const int den = sm + sp - 2 * s0;
        if (den > 0) {
            const float delta = (float)(sm - sp) / (float)(2 * den);
            const float dv = (float)(x0 - xr - (sb - SP_L)) - delta;
            if (dv > 0.f && dv >= P.min_disp && dv <= P.max_disp) d = dv;
        }
    }
    disp[i] = d;
    if (xyz && d == d) {
        // reproject_px's arithmetic (geom.hip) on the float keypoint position: sums left to right in double, out_i = (float)hg_i,
        // then (float)((double)out_i * (1 / hg_3))
        const double v[4] = { (double)(xi + P.x0f), (double)(yi + P.y0f), (double)d, 1.0 };
        double hg[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) s = s + P.Q[r * 4 + k] * v[k];
            hg[r] = s;
        }
        const double ialpha = 1.0 / hg[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float f = (float)hg[r];
            xyz[3 * (size_t)i + r] = (float)((double)f * ialpha);
        }
    }
}

template <int FLAGS>
__global__ void __launch_bounds__(256) k_sparse_match(const int32_t* nl_p, const int32_t* nr_p, int cap,
                                                      const float* __restrict__ xy_l, const int32_t* __restrict__ oct_l, const uint8_t* __restrict__ desc_l,
                                                      const float* __restrict__ xy_r, const int32_t* __restrict__ oct_r, const uint8_t* __restrict__ desc_r,
                                                      int sorted_r, const uint8_t* __restrict__ imgL, const uint8_t* __restrict__ imgR, int stride,
                                                      int cw, int ch, const SparseP P, int32_t* __restrict__ match, float* __restrict__ disp,
                                                      float* __restrict__ xyz, float ratio, uint32_t* claim)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nl = min(*nl_p, cap), nr = min(*nr_p, cap);
    if (i >= nl) return;
    sparse_match_one<FLAGS>(i, lane, nr, xy_l, oct_l, desc_l, xy_r, oct_r, desc_r, sorted_r, imgL, imgR, stride, cw, ch, P, match, disp, xyz,
                            ratio, claim);
}

struct KpSet { float *xy, *size, *angle, *resp; int32_t* oct; uint8_t* desc; };

// One workgroup of 256: the left keypoints whose disparity is a number move, in their order, from the scratch set into the slot (six
// keypoint arrays, descriptors, kp_xyz, kp_disp) and the descriptor of the right keypoint each was associated with goes to dst_rdesc.
// With SP_MUTUAL a keypoint whose winner's claim word names another left keypoint is dropped first (match -1, disparity NaN), and the
// words are put back behind the last read.  rec (pinned, the slot's) = {left keypoints, accepted associations, kept, right
// keypoints} -- the two counts as the extractions left them, so that the host can hold them against the capacity --; n_kp_host = kept.
template <int FLAGS>
__device__ __forceinline__ void sparse_compact_block(int nl_raw, int nr_raw, int cap, const KpSet& src, int32_t* match, float* disp,
                                                     const float* xyz, const uint8_t* __restrict__ desc_r, const KpSet& dst, float* dst_xyz,
                                                     float* dst_disp, uint8_t* dst_rdesc, int32_t* rec, int32_t* n_kp_host, uint32_t* claim,
                                                     int* s_keep, int* s_acc)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nl = min(nl_raw, cap);
    int base = 0, acc = 0;
    for (int i0 = 0; i0 < nl; i0 += 256) {
        const int i = i0 + threadIdx.x;
        float d = 0.f;
        bool keep = false, got = false;
        int m = -1;
        if (i < nl) {
            d = disp[i]; m = match[i];
            if ((FLAGS & SP_MUTUAL) && m >= 0 && (claim[m] & 0xFFFFu) != (unsigned)i) {
                m = -1; d = __builtin_nanf("");
                match[i] = m; disp[i] = d;
            }
            keep = d == d; got = m >= 0;
        }
        const unsigned long long bal = __ballot(keep), bag = __ballot(got);
        if (lane == 0) { s_keep[wv] = __popcll(bal); s_acc[wv] = __popcll(bag); }
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; w++) off += s_keep[w];
        if (keep) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            ((float2*)dst.xy)[pos] = ((const float2*)src.xy)[i];
            dst.size[pos] = src.size[i]; dst.angle[pos] = src.angle[i]; dst.resp[pos] = src.resp[i]; dst.oct[pos] = src.oct[i];
            ((uint4*)dst.desc)[2 * (size_t)pos] = ((const uint4*)src.desc)[2 * (size_t)i];
            ((uint4*)dst.desc)[2 * (size_t)pos + 1] = ((const uint4*)src.desc)[2 * (size_t)i + 1];
            dst_xyz[3 * (size_t)pos] = xyz[3 * (size_t)i]; dst_xyz[3 * (size_t)pos + 1] = xyz[3 * (size_t)i + 1];
            dst_xyz[3 * (size_t)pos + 2] = xyz[3 * (size_t)i + 2];
            dst_disp[pos] = d;
            ((uint4*)dst_rdesc)[2 * (size_t)pos] = ((const uint4*)desc_r)[2 * (size_t)m];
            ((uint4*)dst_rdesc)[2 * (size_t)pos + 1] = ((const uint4*)desc_r)[2 * (size_t)m + 1];
        }
        base += (s_keep[0] + s_keep[1]) + (s_keep[2] + s_keep[3]);
        acc += (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
        __syncthreads();
    }
    if (FLAGS & SP_MUTUAL) {
        const int nr = min(nr_raw, cap);
        for (int j = threadIdx.x; j < nr; j += 256) __hip_atomic_store(claim + j, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(rec + 0, nl_raw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rec + 1, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rec + 2, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rec + 3, nr_raw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(n_kp_host, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

#ifdef VO_SPARSE_TWO_LAUNCHES
template <int FLAGS>
__global__ void __launch_bounds__(256) k_sparse_compact(const int32_t* nl_p, const int32_t* nr_p, int cap, const KpSet src, int32_t* match,
                                                        float* disp, const float* xyz, const uint8_t* __restrict__ desc_r, const KpSet dst,
                                                        float* dst_xyz, float* dst_disp, uint8_t* dst_rdesc, int32_t* rec, int32_t* n_kp_host,
                                                        uint32_t* claim)
{
    __shared__ int s_lds[8];
    sparse_compact_block<FLAGS>(*nl_p, *nr_p, cap, src, match, disp, xyz, desc_r, dst, dst_xyz, dst_disp, dst_rdesc, rec, n_kp_host, claim,
                                s_lds, s_lds + 4);
}
#endif

// Association + refinement (one wave per left keypoint, four to a workgroup) and the compaction in ONE launch.  Every workgroup --
// those whose four keypoints lie beyond nl too -- draws a number at `ticket`; the one that draws the last has seen every other
// arrive and compacts.  Nothing waits and nothing polls.  The hand-off is agent-scope release / acquire in its counter form: every
// wave drains its stores, the workgroup meets, lane 0 releases (fence, then the wait the fence may not carry itself) and adds to the
// ticket; the last arriver acquires, waits, the workgroup meets again and reads match / disp / xyz with plain vector loads.  The
// ticket reads zero before the first launch (sparse_ws_prepare) and the last arriver puts it back.  The claim words of the mutual test
// travel the same way: atomics at agent scope, drained by every wave's wait before the release, read with plain vector loads behind
// the acquire.
template <int FLAGS>
__global__ void __launch_bounds__(256) k_sparse_pair(const int32_t* nl_p, const int32_t* nr_p, int cap, const KpSet src,
                                                     const float* __restrict__ xy_r, const int32_t* __restrict__ oct_r, const uint8_t* __restrict__ desc_r,
                                                     int sorted_r, const uint8_t* __restrict__ imgL, const uint8_t* __restrict__ imgR, int stride,
                                                     int cw, int ch, const SparseP P, int32_t* match, float* disp, float* xyz, const KpSet dst,
                                                     float* dst_xyz, float* dst_disp, uint8_t* dst_rdesc, int32_t* rec, int32_t* n_kp_host,
                                                     int32_t* ticket, float ratio, uint32_t* claim)
{
    __shared__ int s_lds[12];           // ONE LDS object: the compaction's per-wave counts [0 .. 7] and "I am last" [8]
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nl_raw = *nl_p, nr_raw = *nr_p;
    const int nl = min(nl_raw, cap), nr = min(nr_raw, cap);
    if (i < nl)
        sparse_match_one<FLAGS>(i, lane, nr, src.xy, src.oct, src.desc, xy_r, oct_r, desc_r, sorted_r, imgL, imgR, stride, cw, ch, P, match, disp,
                                xyz, ratio, claim);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (int)gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_lds[8] = last;
    }
    __syncthreads();
    if (!s_lds[8]) return;
    sparse_compact_block<FLAGS>(nl_raw, nr_raw, cap, src, match, disp, xyz, desc_r, dst, dst_xyz, dst_disp, dst_rdesc, rec, n_kp_host, claim,
                                s_lds, s_lds + 4);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static int sparse_params(vo_ctx* ctx, float min_disp, float max_disp, float row_tol, int max_hamming, const char* who, SparseP* P)
{
    // (every comparison is false for a NaN: it is refused with the rest)
    if (!(min_disp >= 0.f) || !(max_disp > min_disp) || !(row_tol >= 0.f) || !isfinite(max_disp) || !isfinite(row_tol))
        return vo_fail(ctx, VO_E_ARG, "%s: need 0 <= min_disp < max_disp and row_tol >= 0, all finite", who);
    if (max_hamming < 0 || max_hamming > 256) return vo_fail(ctx, VO_E_ARG, "%s: max_hamming is 0 .. 256", who);
    P->min_disp = min_disp; P->max_disp = max_disp; P->row_tol = row_tol; P->max_hamming = max_hamming;
    for (int o = 0; o < VO_ORB_LEVELS; o++) P->sc[o] = (float)pow((double)1.2f, o);
    for (int k = 0; k < 16; k++) P->Q[k] = 0.0;
    P->x0f = P->y0f = 0.f;
    return VO_OK;
}

// 0 < ratio <= 1 (finite) with VO_SPARSE_RATIO; the ratio of a request without that bit is stored as 0 (it is never read)
static int sparse_assoc_check(vo_ctx* ctx, int flags, float* ratio, const char* who)
{
    if (flags & ~(VO_SPARSE_MUTUAL | VO_SPARSE_RATIO)) return vo_fail(ctx, VO_E_ARG, "%s: association flags %d (bits 0 and 1 only)", who, flags);
    if (!(flags & VO_SPARSE_RATIO)) { *ratio = 0.f; return VO_OK; }
    if (!(*ratio > 0.f) || !(*ratio <= 1.f)) return vo_fail(ctx, VO_E_ARG, "%s: the association ratio must satisfy 0 < ratio <= 1", who);
    return VO_OK;
}

extern "C" int vo_set_sparse_assoc(vo_ctx* ctx, int flags, float ratio)
{
    if (!ctx) return VO_E_ARG;
    if (int rc = sparse_assoc_check(ctx, flags, &ratio, "vo_set_sparse_assoc")) return rc;
    ctx->sp_assoc_flags = flags; ctx->sp_assoc_ratio = ratio;
    return VO_OK;
}

// the one launch of a pair, in the instantiation the request's association tests name
#define SP_PAIR_ARGS(FL) hipLaunchKernelGGL(k_sparse_pair<FL>, dim3(grid), dim3(256), 0, stream, nl_p, nr_p, cap, src, r.kp_xy, r.kp_oct, r.desc, sorted_r, \
                                            imgL, imgR, stride, cw, ch, P, ws.match, ws.disp, ws.xyz, dst, dst_xyz, dst_disp, dst_rdesc, rec, n_kp_host,      \
                                            ws.ticket, ratio, ws.claim)
static void sparse_pair_launch(int flags, float ratio, int grid, hipStream_t stream, const int32_t* nl_p, const int32_t* nr_p, int cap, const KpSet& src,
                               const FrameSlot& r, int sorted_r, const uint8_t* imgL, const uint8_t* imgR, int stride, int cw, int ch, const SparseP& P,
                               SparseWs& ws, const KpSet& dst, float* dst_xyz, float* dst_disp, uint8_t* dst_rdesc, int32_t* rec, int32_t* n_kp_host)
{
    switch (flags & 3) {
    case 0: SP_PAIR_ARGS(0); break;
    case 1: SP_PAIR_ARGS(1); break;
    case 2: SP_PAIR_ARGS(2); break;
    default: SP_PAIR_ARGS(3); break;
    }
}
#undef SP_PAIR_ARGS

static KpSet kp_set(const FrameSlot& f) { return KpSet{ f.kp_xy, f.kp_size, f.kp_angle, f.kp_resp, f.kp_oct, f.desc }; }

int sparse_req_check(vo_ctx* ctx, const SparseReq& q, const char* who)
{
    if (q.nfeatures < 0 || q.nfeatures > ctx->max_kp) return vo_fail(ctx, VO_E_CAP, "nfeatures %d exceeds max_kp %d", q.nfeatures, ctx->max_kp);
    SparseP P;
    if (int rc = sparse_params(ctx, q.min_disp, q.max_disp, q.row_tol, q.max_hamming, who, &P)) return rc;
    float ratio = q.assoc_ratio;
    return sparse_assoc_check(ctx, q.assoc_flags, &ratio, who);
}

static bool sparse_req_same(const SparseReq& a, const SparseReq& b)
{
    // (bit patterns: -0.f and 0.f are two requests, which only costs a recomputation)
    return a.nfeatures == b.nfeatures && a.max_hamming == b.max_hamming && !memcmp(&a.min_disp, &b.min_disp, sizeof(float)) &&
           !memcmp(&a.max_disp, &b.max_disp, sizeof(float)) && !memcmp(&a.row_tol, &b.row_tol, sizeof(float)) &&
           a.assoc_flags == b.assoc_flags && !memcmp(&a.assoc_ratio, &b.assoc_ratio, sizeof(float));
}

void sparse_ws_free(SparseWs& ws)
{
    void* ps[] = { ws.match, ws.disp, ws.xyz, ws.ticket, ws.claim };
    for (void* p : ps) if (p) (void)hipFree(p);
    orb_ws_free(ws.orb_r);
    if (ws.own) {
        for (int k = 0; k < 2; k++) {
            void* ks[] = { ws.own[k].kp_xy, ws.own[k].kp_size, ws.own[k].kp_angle, ws.own[k].kp_resp, ws.own[k].kp_oct, ws.own[k].desc };
            for (void* p : ks) if (p) (void)hipFree(p);
        }
        delete[] ws.own;
    }
    if (ws.own_words) (void)hipHostFree(ws.own_words);
    ws = SparseWs();
}

int sparse_ws_prepare(vo_ctx* ctx, SparseWs& ws, hipStream_t stream, bool own_sets, bool with_orb)
{
    if (ws.ready && (ws.orb_ready || !with_orb)) return VO_OK;
    const size_t cap = (size_t)ctx->kp_cap;
    hipError_t e = hipSuccess;
    auto take = [&](void** p, size_t bytes) { if (e == hipSuccess && !*p) e = hipMalloc(p, bytes + 256); };
    if (own_sets && !ws.own) {
        ws.own = new FrameSlot[2];
        if (hipHostMalloc((void**)&ws.own_words, 64, hipHostMallocDefault) != hipSuccess) e = hipErrorOutOfMemory;
        else memset(ws.own_words, 0, 64);
        for (int k = 0; k < 2 && e == hipSuccess; k++) {
            FrameSlot& s = ws.own[k];
            take((void**)&s.kp_xy, cap * 8); take((void**)&s.kp_size, cap * 4); take((void**)&s.kp_angle, cap * 4);
            take((void**)&s.kp_resp, cap * 4); take((void**)&s.kp_oct, cap * 4); take((void**)&s.desc, cap * 32);
            s.n_kp_host = ws.own_words + 8 * k;
        }
        ws.l = &ws.own[0]; ws.r = &ws.own[1];
    }
    if (e == hipSuccess && with_orb && !ws.orb_ready && orb_ws_alloc(ctx, ws.orb_r)) e = hipErrorOutOfMemory;
    take((void**)&ws.match, cap * 4); take((void**)&ws.disp, cap * 4); take((void**)&ws.xyz, cap * 12);
    take((void**)&ws.ticket, 64); take((void**)&ws.claim, cap * 4);
    // the ticket must read zero, and every claim word 0xFFFFFFFF, before the first launch on WHATEVER stream that is: set on that
    // stream, and waited for
    if (e == hipSuccess && !ws.ready) {
        e = hipMemsetAsync(ws.ticket, 0, 64, stream);
        if (e == hipSuccess) e = hipMemsetAsync(ws.claim, 0xFF, cap * 4, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    if (e != hipSuccess) {
        FrameSlot *l = ws.l, *r = ws.r;
        const bool borrowed = !ws.own;
        sparse_ws_free(ws);
        if (borrowed) { ws.l = l; ws.r = r; }
        return vo_fail(ctx, VO_E_HIP, "sparse stereo scratch: allocation failed: %s", hipGetErrorString(e));
    }
    ws.ready = true;
    if (with_orb) ws.orb_ready = true;
    return VO_OK;
}

int sparse_enqueue(vo_ctx* ctx, FrameSlot& f, SparseWs& ws, const SparseReq& q)
{
    SparseP P;
    if (int rcp = sparse_params(ctx, q.min_disp, q.max_disp, q.row_tol, q.max_hamming, "sparse stereo", &P)) return rcp;
    int x0 = 0, y0 = 0, x1 = f.w, y1 = f.h;
    if (ctx->has_roi) { x0 = ctx->roi[0]; y0 = ctx->roi[1]; x1 = ctx->roi[2] < f.w ? ctx->roi[2] : f.w; y1 = ctx->roi[3] < f.h ? ctx->roi[3] : f.h; }
    const int cw = x1 - x0, ch = y1 - y0;
    if (cw <= 2 * VO_ORB_EDGE || ch <= 2 * VO_ORB_EDGE || x0 < 0 || y0 < 0) {
        // No pixel inside ORB's border: no keypoint on either side, nothing to launch.  The one place this function waits: a voided
        // earlier run into the slot (the stream is ordered behind it) may still be writing the record the host clears here.  The
        // scratch sets' count words are left alone (an engine's earlier pair may still be reading them).
        VO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        f.sp_rec[0] = f.sp_rec[1] = f.sp_rec[2] = f.sp_rec[3] = 0;
        *f.n_kp_host = 0;
        return VO_OK;
    }
    FrameSlot &sl = *ws.l, &sr = *ws.r;
    const size_t off = (size_t)y0 * f.w + x0;
    // the left crop rectangle on BOTH images (columns compare directly), the two extractions as one batch: one launch per kernel
    const OrbIn in[2] = { { &sl, ctx->orbws, f.left + off, nullptr, nullptr, f.w, 0, 0 }, { &sr, &ws.orb_r, f.right + off, nullptr, nullptr, f.w, 0, 0 } };
    if (int rc = orb_enqueue_jobs(ctx, in, 2, cw, ch, q.nfeatures, 0, 0, 0)) return rc;
    memcpy(P.Q, ctx->Q, sizeof(P.Q));
    P.x0f = (float)x0; P.y0f = (float)y0;
    StageTimer t(ctx, VO_T_MATCH);
#ifdef VO_SPARSE_TWO_LAUNCHES
#define SP_TWO(FL)                                                                                                                                   \
    do {                                                                                                                                              \
        hipLaunchKernelGGL(k_sparse_match<FL>, dim3(div_up(ctx->kp_cap, 4)), dim3(256), 0, ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap,      \
                           sl.kp_xy, sl.kp_oct, sl.desc, sr.kp_xy, sr.kp_oct, sr.desc, 1, f.left + off, f.right + off, f.w, cw, ch, P,                 \
                           ws.match, ws.disp, ws.xyz, q.assoc_ratio, ws.claim);                                                                       \
        VO_CHECK_LAUNCH(ctx);                                                                                                                         \
        hipLaunchKernelGGL(k_sparse_compact<FL>, dim3(1), dim3(256), 0, ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap, kp_set(sl), ws.match,   \
                           ws.disp, ws.xyz, sr.desc, kp_set(f), f.kp_xyz, f.kp_disp, f.kp_rdesc, f.sp_rec, f.n_kp_host, ws.claim);                    \
    } while (0)
    switch (q.assoc_flags & 3) {
    case 0: SP_TWO(0); break;
    case 1: SP_TWO(1); break;
    case 2: SP_TWO(2); break;
    default: SP_TWO(3); break;
    }
#undef SP_TWO
#else
    sparse_pair_launch(q.assoc_flags, q.assoc_ratio, div_up(ctx->kp_cap, 4), ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap, kp_set(sl), sr, 1,
                       f.left + off, f.right + off, f.w, cw, ch, P, ws, kp_set(f), f.kp_xyz, f.kp_disp, f.kp_rdesc, f.sp_rec, f.n_kp_host);
#endif
    VO_CHECK_LAUNCH(ctx);
    return VO_OK;
}

// the chain into the slot has finished and the host has waited for it: today's checks from the slot's record, then the slot's state
static int sparse_collect(vo_ctx* ctx, FrameSlot& f, int32_t* counts3, int assoc_flags)
{
    const volatile int32_t* rec = f.sp_rec;
    const int nl = rec[0], nr = rec[3];
    if (nl > ctx->kp_cap || nr > ctx->kp_cap)
        return vo_fail(ctx, VO_E_CAP, "%d / %d keypoints (response ties included) exceed capacity %d; raise max_kp", nl, nr, ctx->kp_cap);
    if (nr > 65535) return vo_fail(ctx, VO_E_CAP, "vo_sparse_stereo: %d right keypoints (at most 65535)", nr);
    if ((assoc_flags & VO_SPARSE_MUTUAL) && nl > 65535)
        return vo_fail(ctx, VO_E_CAP, "vo_sparse_stereo: %d left keypoints with the mutual test (at most 65535)", nl);
    counts3[0] = rec[0]; counts3[1] = rec[1]; counts3[2] = rec[2];
    f.n_kp = rec[2];
    f.has_kp = true; f.kp_depth = true;
    return VO_OK;
}

extern "C" int vo_sparse_stereo(vo_ctx* ctx, int slot, int nfeatures, float min_disp, float max_disp, float row_tol, int max_hamming,
                                int32_t* counts3)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || !counts3) return vo_fail(ctx, VO_E_ARG, "vo_sparse_stereo: bad argument");
    const SparseReq q = { nfeatures, min_disp, max_disp, row_tol, max_hamming, ctx->sp_assoc_flags, ctx->sp_assoc_ratio };
    if (int rcq = sparse_req_check(ctx, q, "vo_sparse_stereo")) return rcq;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_pair) return vo_fail(ctx, VO_E_STATE, "slot %d holds no image pair", slot);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    const bool same = sparse_req_same(q, f.sp_req);
    if (f.sp_pending && same) {
        // a look-ahead engine ran the whole chain: wait for it, nothing to launch
        f.sp_pending = false;
        VO_HIP(ctx, hipEventSynchronize(f.ready));
        if (f.pending && f.counted && ctx->inflight > 0) ctx->inflight--;
        f.pending = false; f.counted = false;
        if ((rc = sparse_collect(ctx, f, counts3, q.assoc_flags))) return rc;
        f.sp_ahead = true;
        return VO_OK;
    }
    if (slot_sparse(f) && f.sp_ahead && same) {
        // a slot begun ahead and already collected with this request (e.g. ahead of a pose step): its counts again.  A result
        // computed synchronously is never reused: the synchronous call recomputes, as it always has
        if ((rc = slot_wait(ctx, f))) return rc;
        counts3[0] = f.sp_rec[0]; counts3[1] = f.sp_rec[1]; counts3[2] = f.sp_rec[2];
        return VO_OK;
    }
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;     // (steps begun ahead may still read the slot's keypoints)
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false; f.sp_pending = false; f.sp_ahead = false;
    f.mono_serial = 0;              // depths of a monocular pose step belong to the keypoints this call replaces (as orb_enqueue)
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;     // no ORB extraction ever asks for these: the next one recomputes
    counts3[0] = counts3[1] = counts3[2] = 0;
    if ((rc = sparse_ws_prepare(ctx, ctx->sp_main, ctx->stream, false))) return rc;
    if ((rc = sparse_enqueue(ctx, f, ctx->sp_main, q))) return rc;
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the one synchronisation
    f.sp_req = q;
    return sparse_collect(ctx, f, counts3, q.assoc_flags);
}

extern "C" int vo_download_keypoint_depth(vo_ctx* ctx, int slot, float* xyz, float* disp, int cap, int* n_out)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS) return vo_fail(ctx, VO_E_ARG, "vo_download_keypoint_depth: bad slot");
    FrameSlot& f = ctx->slots[slot];
    if (!slot_sparse(f)) return vo_fail(ctx, VO_E_STATE, "slot %d: the keypoints carry no depth (vo_sparse_stereo)", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, f); if (rcw) return rcw; }
    const int n = f.n_kp;
    if (n_out) *n_out = n;
    if (n == 0 || (!xyz && !disp)) return VO_OK;
    if (n > cap) return vo_fail(ctx, VO_E_CAP, "%d keypoints exceed the output capacity %d", n, cap);
    int rc = VO_OK;
    if (xyz) rc = xfer_d2h(ctx, xyz, f.kp_xyz, (size_t)n * 12);
    if (disp && !rc) rc = xfer_d2h(ctx, disp, f.kp_disp, (size_t)n * 4);
    if (rc) return rc;
    return xfer_flush(ctx);
}

extern "C" int vo_download_keypoint_rdesc(vo_ctx* ctx, int slot, uint8_t* rdesc, int cap, int* n_out)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS) return vo_fail(ctx, VO_E_ARG, "vo_download_keypoint_rdesc: bad slot");
    FrameSlot& f = ctx->slots[slot];
    if (!slot_sparse(f)) return vo_fail(ctx, VO_E_STATE, "slot %d: the keypoints carry no depth (vo_sparse_stereo)", slot);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, f); if (rcw) return rcw; }
    const int n = f.n_kp;
    if (n_out) *n_out = n;
    if (n == 0 || !rdesc) return VO_OK;
    if (n > cap) return vo_fail(ctx, VO_E_CAP, "%d keypoints exceed the output capacity %d", n, cap);
    if (int rc = xfer_d2h(ctx, rdesc, f.kp_rdesc, (size_t)n * 32)) return rc;
    return xfer_flush(ctx);
}

extern "C" int vo_sparse_match_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l,
                                    const int32_t* oct_l, const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r,
                                    const uint8_t* desc_r, int nr, float min_disp, float max_disp, float row_tol, int max_hamming,
                                    int32_t* match_out, float* disp_out)
{
    if (!ctx || !left || !right || w <= 0 || h <= 0 || nl < 0 || nr < 0) return vo_fail(ctx, VO_E_ARG, "vo_sparse_match_host: bad argument");
    if (w > ctx->max_w || h > ctx->max_h) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context", w, h);
    if (nr > 65535) return vo_fail(ctx, VO_E_CAP, "vo_sparse_match_host: %d right keypoints (at most 65535)", nr);
    if (nl > ctx->kp_cap || nr > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "%d / %d keypoints exceed capacity %d", nl, nr, ctx->kp_cap);
    if ((nl > 0 && (!xy_l || !oct_l || !desc_l || !match_out || !disp_out)) || (nr > 0 && (!xy_r || !oct_r || !desc_r)))
        return vo_fail(ctx, VO_E_ARG, "vo_sparse_match_host: null pointer");
    SparseP P;
    if (int rcp = sparse_params(ctx, min_disp, max_disp, row_tol, max_hamming, "vo_sparse_match_host", &P)) return rcp;
    for (int i = 0; i < nl; i++) if (oct_l[i] < 0 || oct_l[i] >= VO_ORB_LEVELS) return vo_fail(ctx, VO_E_ARG, "vo_sparse_match_host: octave %d", oct_l[i]);
    int sorted_r = 1;
    for (int j = 0; j < nr; j++) {
        if (oct_r[j] < 0 || oct_r[j] >= VO_ORB_LEVELS) return vo_fail(ctx, VO_E_ARG, "vo_sparse_match_host: octave %d", oct_r[j]);
        if (j && oct_r[j] < oct_r[j - 1]) sorted_r = 0;
    }
    if (nl == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcw = sparse_ws_prepare(ctx, ctx->sp_main, ctx->stream, false, false)) return rcw;
    FrameSlot& sl = ctx->slots[VO_NUM_SLOTS];
    FrameSlot& sr = ctx->sparse_r;
    const size_t npx = (size_t)w * h;
    VO_HIP(ctx, hipMemcpyAsync(sl.left, left, npx, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(sl.right, right, npx, hipMemcpyHostToDevice, ctx->stream));
    int rc = xfer_h2d(ctx, sl.kp_xy, xy_l, (size_t)nl * 8);
    if (!rc) rc = xfer_h2d(ctx, sl.kp_oct, oct_l, (size_t)nl * 4);
    if (!rc) rc = xfer_h2d(ctx, sl.desc, desc_l, (size_t)nl * 32);
    if (!rc) rc = xfer_h2d(ctx, sr.kp_xy, xy_r, (size_t)nr * 8);
    if (!rc) rc = xfer_h2d(ctx, sr.kp_oct, oct_r, (size_t)nr * 4);
    if (!rc) rc = xfer_h2d(ctx, sr.desc, desc_r, (size_t)nr * 32);
    if (rc) return rc;
    sl.has_kp = false; sl.kp_depth = false;
    *sl.n_kp_host = nl; *sr.n_kp_host = nr;
    hipLaunchKernelGGL(k_sparse_match<0>, dim3(div_up(nl, 4)), dim3(256), 0, ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap, sl.kp_xy, sl.kp_oct,
                       sl.desc, sr.kp_xy, sr.kp_oct, sr.desc, sorted_r, sl.left, sl.right, w, w, h, P, ctx->sp_main.match, ctx->sp_main.disp, (float*)nullptr,
                       0.f, (uint32_t*)nullptr);
    VO_CHECK_LAUNCH(ctx);
    rc = xfer_d2h(ctx, match_out, ctx->sp_main.match, (size_t)nl * 4);
    if (!rc) rc = xfer_d2h(ctx, disp_out, ctx->sp_main.disp, (size_t)nl * 4);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// k_sparse_pair alone on host arrays (the seam its tests use): vo_sparse_match_host's inputs plus Q and the ROI origin; the survivors
// are compacted from the scratch set into a destination of their own (never the source) and come back with their disparity and 3-D
// point.  The scratch set's size / angle / response are whatever an earlier call left there: they travel, nobody reads them.
// The association tests are arguments here: the context's state is neither read nor changed.
extern "C" int vo_sparse_pair_host_ex(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l,
                                   const int32_t* oct_l, const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r,
                                   const uint8_t* desc_r, int nr, float min_disp, float max_disp, float row_tol, int max_hamming,
                                   int assoc_flags, float assoc_ratio, const double* Q16, int roi_x0, int roi_y0, int32_t* match_out,
                                   float* disp_out, float* kp_xy, int32_t* kp_octave, uint8_t* desc, float* kp_disp, float* kp_xyz,
                                   uint8_t* kp_rdesc, int32_t* counts3)
{
    if (!ctx || !left || !right || w <= 0 || h <= 0 || nl < 0 || nr < 0 || !Q16 || !counts3) return vo_fail(ctx, VO_E_ARG, "vo_sparse_pair_host: bad argument");
    if (w > ctx->max_w || h > ctx->max_h) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context", w, h);
    if (nr > 65535) return vo_fail(ctx, VO_E_CAP, "vo_sparse_pair_host: %d right keypoints (at most 65535)", nr);
    if (nl > ctx->kp_cap || nr > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "%d / %d keypoints exceed capacity %d", nl, nr, ctx->kp_cap);
    if (int rca = sparse_assoc_check(ctx, assoc_flags, &assoc_ratio, "vo_sparse_pair_host")) return rca;
    if ((assoc_flags & VO_SPARSE_MUTUAL) && nl > 65535) return vo_fail(ctx, VO_E_CAP, "vo_sparse_pair_host: %d left keypoints with the mutual test (at most 65535)", nl);
    if ((nl > 0 && (!xy_l || !oct_l || !desc_l || !match_out || !disp_out || !kp_xy || !kp_octave || !desc || !kp_disp || !kp_xyz)) ||
        (nr > 0 && (!xy_r || !oct_r || !desc_r)))
        return vo_fail(ctx, VO_E_ARG, "vo_sparse_pair_host: null pointer");
    SparseP P;
    if (int rcp = sparse_params(ctx, min_disp, max_disp, row_tol, max_hamming, "vo_sparse_pair_host", &P)) return rcp;
    for (int i = 0; i < nl; i++) if (oct_l[i] < 0 || oct_l[i] >= VO_ORB_LEVELS) return vo_fail(ctx, VO_E_ARG, "vo_sparse_pair_host: octave %d", oct_l[i]);
    int sorted_r = 1;
    for (int j = 0; j < nr; j++) {
        if (oct_r[j] < 0 || oct_r[j] >= VO_ORB_LEVELS) return vo_fail(ctx, VO_E_ARG, "vo_sparse_pair_host: octave %d", oct_r[j]);
        if (j && oct_r[j] < oct_r[j - 1]) sorted_r = 0;
    }
    memcpy(P.Q, Q16, sizeof(P.Q));
    P.x0f = (float)roi_x0; P.y0f = (float)roi_y0;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcw = sparse_ws_prepare(ctx, ctx->sp_main, ctx->stream, false, false)) return rcw;
    SparseWs& ws = ctx->sp_main;
    FrameSlot& sl = ctx->slots[VO_NUM_SLOTS];
    FrameSlot& sr = ctx->sparse_r;
    // the destination: one allocation cut into the keypoint arrays (a test seam: allocated and freed per call)
    const size_t cap = ((size_t)ctx->kp_cap + 63) & ~(size_t)63;
    uint8_t* d = nullptr;
    VO_HIP(ctx, hipMalloc((void**)&d, cap * (8 + 4 + 4 + 4 + 4 + 32 + 12 + 4 + 32) + 256));
    KpSet dst;
    dst.xy = (float*)d; dst.size = (float*)(d + cap * 8); dst.angle = (float*)(d + cap * 12); dst.resp = (float*)(d + cap * 16);
    dst.oct = (int32_t*)(d + cap * 20); dst.desc = d + cap * 24;
    float* const dst_xyz = (float*)(d + cap * 56);
    float* const dst_disp = (float*)(d + cap * 68);
    uint8_t* const dst_rdesc = d + cap * 72;
    const size_t npx = (size_t)w * h;
    int rc = VO_OK;
    do {
        if (hipMemcpyAsync(sl.left, left, npx, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(sl.right, right, npx, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = vo_fail(ctx, VO_E_HIP, "vo_sparse_pair_host: upload failed"); break; }
        if ((rc = xfer_h2d(ctx, sl.kp_xy, xy_l, (size_t)nl * 8))) break;
        if ((rc = xfer_h2d(ctx, sl.kp_oct, oct_l, (size_t)nl * 4))) break;
        if ((rc = xfer_h2d(ctx, sl.desc, desc_l, (size_t)nl * 32))) break;
        if ((rc = xfer_h2d(ctx, sr.kp_xy, xy_r, (size_t)nr * 8))) break;
        if ((rc = xfer_h2d(ctx, sr.kp_oct, oct_r, (size_t)nr * 4))) break;
        if ((rc = xfer_h2d(ctx, sr.desc, desc_r, (size_t)nr * 32))) break;
        sl.has_kp = false; sl.kp_depth = false;
        *sl.n_kp_host = nl; *sr.n_kp_host = nr;
        // (the product's grid: every workgroup draws a ticket, most of them with no keypoint of their own)
        sparse_pair_launch(assoc_flags, assoc_ratio, div_up(ctx->kp_cap, 4), ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap, kp_set(sl), sr,
                           sorted_r, sl.left, sl.right, w, w, h, P, ws, dst, dst_xyz, dst_disp, dst_rdesc, sl.sp_rec, sl.n_kp_host);
        if (hipGetLastError() != hipSuccess) { rc = vo_fail(ctx, VO_E_HIP, "vo_sparse_pair_host: launch failed"); break; }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = vo_fail(ctx, VO_E_HIP, "vo_sparse_pair_host: the launch failed"); break; }
        const volatile int32_t* rec = sl.sp_rec;
        counts3[0] = rec[0]; counts3[1] = rec[1]; counts3[2] = rec[2];
        const int n = rec[2];
        if (n < 0 || n > nl) { rc = vo_fail(ctx, VO_E_STATE, "vo_sparse_pair_host: %d survivors of %d keypoints", n, nl); break; }
        if ((rc = xfer_d2h(ctx, match_out, ws.match, (size_t)nl * 4))) break;
        if ((rc = xfer_d2h(ctx, disp_out, ws.disp, (size_t)nl * 4))) break;
        if ((rc = xfer_d2h(ctx, kp_xy, dst.xy, (size_t)n * 8))) break;
        if ((rc = xfer_d2h(ctx, kp_octave, dst.oct, (size_t)n * 4))) break;
        if ((rc = xfer_d2h(ctx, desc, dst.desc, (size_t)n * 32))) break;
        if ((rc = xfer_d2h(ctx, kp_disp, dst_disp, (size_t)n * 4))) break;
        if ((rc = xfer_d2h(ctx, kp_xyz, dst_xyz, (size_t)n * 12))) break;
        if (kp_rdesc && (rc = xfer_d2h(ctx, kp_rdesc, dst_rdesc, (size_t)n * 32))) break;
        rc = xfer_flush(ctx);
    } while (0);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    return rc;
}

extern "C" int vo_sparse_pair_host(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, const float* xy_l,
                                   const int32_t* oct_l, const uint8_t* desc_l, int nl, const float* xy_r, const int32_t* oct_r,
                                   const uint8_t* desc_r, int nr, float min_disp, float max_disp, float row_tol, int max_hamming,
                                   const double* Q16, int roi_x0, int roi_y0, int32_t* match_out, float* disp_out, float* kp_xy,
                                   int32_t* kp_octave, uint8_t* desc, float* kp_disp, float* kp_xyz, int32_t* counts3)
{
    return vo_sparse_pair_host_ex(ctx, left, right, w, h, xy_l, oct_l, desc_l, nl, xy_r, oct_r, desc_r, nr, min_disp, max_disp, row_tol, max_hamming,
                                  0, 0.f, Q16, roi_x0, roi_y0, match_out, disp_out, kp_xy, kp_octave, desc, kp_disp, kp_xyz, nullptr, counts3);
}
