// Sparse stereo depth on gfx950: per-keypoint disparity from left / right ORB, no dense disparity image.
// NOT part of the reference (openVO reads a dense SGBM disparity at its keypoints, stereo_odometer.py:50-79,117): defined by this
// build, see include/vo355.h (vo_sparse_stereo) and tests/sparse_stereo_ref.py, which restates it in numpy.
//   k_sparse_match     one wave per left keypoint: association along the epipolar row (lanes over right keypoints, wave argmin
//                      on (distance << 16 | j)), then the sub-pixel refinement by 11 x 11 SAD over 11 shifts and the 3-D point
//   k_sparse_compact   ordered compaction (ballot prefix) of the surviving left keypoints from the scratch set into the slot
// Compiled with -ffp-contract=off like the rest of the library: the float32 / float64 arithmetic below is the definition.
#include <math.h>
#include "vo_internal.h"

#define SP_W 5     // half width of the SAD window (11 x 11)
#define SP_L 5     // shifts -L .. L around the associated right keypoint

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
__global__ void __launch_bounds__(256) k_sparse_match(const int32_t* nl_p, const int32_t* nr_p, int cap,
                                                      const float* __restrict__ xy_l, const int32_t* __restrict__ oct_l, const uint8_t* __restrict__ desc_l,
                                                      const float* __restrict__ xy_r, const int32_t* __restrict__ oct_r, const uint8_t* __restrict__ desc_r,
                                                      int sorted_r, const uint8_t* __restrict__ imgL, const uint8_t* __restrict__ imgR, int stride,
                                                      int cw, int ch, const SparseP P, int32_t* __restrict__ match, float* __restrict__ disp,
                                                      float* __restrict__ xyz)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nl = min(*nl_p, cap), nr = min(*nr_p, cap);
    if (i >= nl) return;
    const float nanf_ = __builtin_nanf("");
    const float xi = xy_l[2 * i], yi = xy_l[2 * i + 1];
    const int oi = oct_l[i];
    unsigned key = 0xFFFFFFFFu;
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
            key = min(key, ((unsigned)dist << 16) | (unsigned)j);
        }
        key = sp_wave_min_u32(key);
    }
    if (key == 0xFFFFFFFFu || (int)(key >> 16) > P.max_hamming) {         // (wave-uniform from here on)
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

struct KpSet { float *xy, *size, *angle, *resp; int32_t* oct; uint8_t* desc; };

// One block: the left keypoints whose disparity is a number move, in their order, from the scratch set into the slot (six keypoint
// arrays, descriptors, kp_xyz, kp_disp).  rec (pinned) = {left keypoints, accepted associations, kept}; n_kp_host = kept.
__global__ void __launch_bounds__(256) k_sparse_compact(const int32_t* nl_p, int cap, const KpSet src, const int32_t* __restrict__ match,
                                                        const float* __restrict__ disp, const float* __restrict__ xyz, const KpSet dst,
                                                        float* __restrict__ dst_xyz, float* __restrict__ dst_disp, int32_t* rec,
                                                        int32_t* n_kp_host)
{
    __shared__ int s_keep[4], s_acc[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nl = min(*nl_p, cap);
    int base = 0, acc = 0;
    for (int i0 = 0; i0 < nl; i0 += 256) {
        const int i = i0 + threadIdx.x;
        float d = 0.f;
        bool keep = false, got = false;
        if (i < nl) { d = disp[i]; keep = d == d; got = match[i] >= 0; }
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
        }
        base += (s_keep[0] + s_keep[1]) + (s_keep[2] + s_keep[3]);
        acc += (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(rec + 0, nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rec + 1, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rec + 2, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(n_kp_host, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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

static KpSet kp_set(const FrameSlot& f) { return KpSet{ f.kp_xy, f.kp_size, f.kp_angle, f.kp_resp, f.kp_oct, f.desc }; }

extern "C" int vo_sparse_stereo(vo_ctx* ctx, int slot, int nfeatures, float min_disp, float max_disp, float row_tol, int max_hamming,
                                int32_t* counts3)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || !counts3) return vo_fail(ctx, VO_E_ARG, "vo_sparse_stereo: bad argument");
    if (nfeatures < 0 || nfeatures > ctx->max_kp) return vo_fail(ctx, VO_E_CAP, "nfeatures %d exceeds max_kp %d", nfeatures, ctx->max_kp);
    SparseP P;
    if (int rcp = sparse_params(ctx, min_disp, max_disp, row_tol, max_hamming, "vo_sparse_stereo", &P)) return rcp;
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_pair) return vo_fail(ctx, VO_E_STATE, "slot %d holds no image pair", slot);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = slot_wait(ctx, f)) || (rc = slot_before_overwrite(ctx, f))) return rc;     // (steps begun ahead may still read the slot's keypoints)
    f.has_kp = false; f.kp_depth = false; f.kp_pending = false;
    f.mono_serial = 0;              // depths of a monocular pose step belong to the keypoints this call replaces (as orb_enqueue)
    f.kp_params[0] = f.kp_params[1] = f.kp_params[2] = f.kp_params[3] = -1;     // no ORB extraction ever asks for these: the next one recomputes
    counts3[0] = counts3[1] = counts3[2] = 0;
    int x0 = 0, y0 = 0, x1 = f.w, y1 = f.h;
    if (ctx->has_roi) { x0 = ctx->roi[0]; y0 = ctx->roi[1]; x1 = ctx->roi[2] < f.w ? ctx->roi[2] : f.w; y1 = ctx->roi[3] < f.h ? ctx->roi[3] : f.h; }
    const int cw = x1 - x0, ch = y1 - y0;
    if (cw <= 0 || ch <= 0 || x0 < 0 || y0 < 0) { *f.n_kp_host = 0; f.n_kp = 0; f.has_kp = true; f.kp_depth = true; return VO_OK; }
    FrameSlot& sl = ctx->slots[VO_NUM_SLOTS];
    FrameSlot& sr = ctx->sparse_r;
    const size_t off = (size_t)y0 * f.w + x0;
    // the left crop rectangle on BOTH images: columns compare directly
    if ((rc = orb_enqueue(ctx, &sl, f.left + off, f.w, cw, ch, nfeatures, 0, nullptr, 0, 0, 0, nullptr, 0))) return rc;
    if ((rc = orb_enqueue(ctx, &sr, f.right + off, f.w, cw, ch, nfeatures, 0, nullptr, 0, 0, 0, nullptr, 0))) return rc;
    memcpy(P.Q, ctx->Q, sizeof(P.Q));
    P.x0f = (float)x0; P.y0f = (float)y0;
    {
        StageTimer t(ctx, VO_T_MATCH);
        hipLaunchKernelGGL(k_sparse_match, dim3(div_up(ctx->kp_cap, 4)), dim3(256), 0, ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap,
                           sl.kp_xy, sl.kp_oct, sl.desc, sr.kp_xy, sr.kp_oct, sr.desc, 1, f.left + off, f.right + off, f.w, cw, ch, P,
                           ctx->sp_match, ctx->sp_disp, ctx->sp_xyz);
        VO_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_sparse_compact, dim3(1), dim3(256), 0, ctx->stream, sl.n_kp_host, ctx->kp_cap, kp_set(sl), ctx->sp_match, ctx->sp_disp,
                           ctx->sp_xyz, kp_set(f), f.kp_xyz, f.kp_disp, ctx->sp_rec, f.n_kp_host);
        VO_CHECK_LAUNCH(ctx);
    }
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the one synchronisation
    const int nl = *(volatile int32_t*)sl.n_kp_host, nr = *(volatile int32_t*)sr.n_kp_host;
    if (nl > ctx->kp_cap || nr > ctx->kp_cap)
        return vo_fail(ctx, VO_E_CAP, "%d / %d keypoints (response ties included) exceed capacity %d; raise max_kp", nl, nr, ctx->kp_cap);
    if (nr > 65535) return vo_fail(ctx, VO_E_CAP, "vo_sparse_stereo: %d right keypoints (at most 65535)", nr);
    const volatile int32_t* rec = ctx->sp_rec;
    counts3[0] = rec[0]; counts3[1] = rec[1]; counts3[2] = rec[2];
    f.n_kp = rec[2];
    f.has_kp = true; f.kp_depth = true;
    return VO_OK;
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
    hipLaunchKernelGGL(k_sparse_match, dim3(div_up(nl, 4)), dim3(256), 0, ctx->stream, sl.n_kp_host, sr.n_kp_host, ctx->kp_cap, sl.kp_xy, sl.kp_oct,
                       sl.desc, sr.kp_xy, sr.kp_oct, sr.desc, sorted_r, sl.left, sl.right, w, w, h, P, ctx->sp_match, ctx->sp_disp, (float*)nullptr);
    VO_CHECK_LAUNCH(ctx);
    rc = xfer_d2h(ctx, match_out, ctx->sp_match, (size_t)nl * 4);
    if (!rc) rc = xfer_d2h(ctx, disp_out, ctx->sp_disp, (size_t)nl * 4);
    if (rc) return rc;
    return xfer_flush(ctx);
}
