// Dense direct alignment (include/vo355.h, vo_direct_align): NOT part of the reference, defined by this build operation by
// operation; tests/direct_ref.py restates it.
//   k_direct_align   ONE launch of ONE workgroup for all levels and iterations, in the manner of k_pnp_finish: thread t owns the
//                    lattice points with linear index = t modulo the block size, ascending; selection and the 3-D point are
//                    recomputed per iteration (six byte / short loads that hit the cache: nothing is packed, no scratch memory);
//                    every thread keeps the 29 sums of an iteration in float64 registers, a DPP tree sums the wave, the waves'
//                    values go through LDS and are added in wave order (one sum per thread of the first 29), thread 0 solves
//                    (pn_solve6) and updates the pose in LDS (pn_apply_twist) behind a barrier.  Nothing is handed between workgroups: no atomics, no tickets, no waiting;
//                    every loop is bounded by levels x iters x lattice; every read lies inside the level rectangle by construction
//                    (lattice points keep one pixel off its edges, a participating sample has floor(u) + 1 <= x_hi - 1).
// and the host side: the pyramids by klt.hip's launcher into the Lucas-Kanade workspace, the lattice steps, the checks.
#include <math.h>
#include "vo_internal.h"
#include "pn_solve.h"

#define VO_DIRECT_BLOCK 512

struct DirectLevel {
    const uint8_t *A, *B;               // level images of slot a / slot b, stride w
    int w, x_lo, x_hi, y_lo, y_hi, s, nx, n;   // n = nx ny lattice points
    double fx, fy, cx, cy;
};
struct DirectPrm {
    DirectLevel lv[VO_DIRECT_MAX_LEVELS];
    const int16_t* disp16;              // slot a, level 0, stride w0
    int w0, levels, iters, min_pixels, g2min;
    double d16_lo, d16_hi, huber, z_min, q03, q13, q23, q32, q33;
    double Rt0[12];
};

// The end of an iteration in one lane: S = the 29 sums of the block (LDS), sel = the waves' selected counts.  Fills the level's
// record, then stops the step (status 2: starved, -1: a value that is not finite or a pivot that is not positive) or solves,
// updates the pose and keeps the sums as those of the last completed linearisation.
__device__ __noinline__ void direct_step(const double* S, const int* sel, int nw, bool first, int min_pixels, double* pose, double* last,
                                         vo_direct_level* lv, int* status, int* done)
{
    const int n = (int)S[27];
    if (first) {
        int nsel = 0;
        for (int q = 0; q < nw; q++) nsel += sel[q];
        lv->selected = nsel; lv->n_first = n; lv->wr2_first = S[28];
    }
    lv->n_last = n; lv->wr2_last = S[28];
    if (n < min_pixels) { *status = 2; return; }
    double H[21], g[6], d[6] = { 0, 0, 0, 0, 0, 0 };
    bool ok = isfinite(S[28]);
#pragma unroll
    for (int k = 0; k < 21; k++) { H[k] = S[k]; ok = ok && isfinite(H[k]); }
#pragma unroll
    for (int k = 0; k < 6; k++) { g[k] = S[21 + k]; ok = ok && isfinite(g[k]); }
    ok = ok && pn_solve6(H, g, d);
    double Rn[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Rn[k] = pose[k];
    if (ok) pn_apply_twist(Rn, d);
#pragma unroll
    for (int k = 0; k < 12; k++) ok = ok && isfinite(Rn[k]);
    if (!ok) { *status = -1; return; }
#pragma unroll
    for (int k = 0; k < 12; k++) pose[k] = Rn[k];
    for (int k = 0; k < 29; k++) last[k] = S[k];
    *done = *done + 1;
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_direct_align(DirectPrm P, vo_direct_rec* __restrict__ rec)
{
    constexpr int NW = BLOCK / 64;
    __shared__ double s_red[NW][29], s_sum[29], s_pose[12], s_last[29];
    __shared__ int s_sel[NW], s_status, s_done;
    __shared__ vo_direct_level s_lv[VO_DIRECT_MAX_LEVELS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        for (int k = 0; k < 12; k++) s_pose[k] = P.Rt0[k];
        for (int k = 0; k < 29; k++) s_last[k] = 0.0;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) {
            s_lv[l].s = l < P.levels ? P.lv[l].s : 0;
            s_lv[l].selected = s_lv[l].n_first = s_lv[l].n_last = 0;
            s_lv[l].wr2_first = s_lv[l].wr2_last = 0.0;
        }
        s_status = 0; s_done = 0;
    }
    __syncthreads();
    bool stop = false;
    for (int L = P.levels - 1; L >= 0 && !stop; --L) {
        const DirectLevel lv = P.lv[L];
        const uint8_t* __restrict__ A = lv.A;
        const uint8_t* __restrict__ B = lv.B;
        const double xlo = (double)lv.x_lo, xhi1 = (double)(lv.x_hi - 1), ylo = (double)lv.y_lo, yhi1 = (double)(lv.y_hi - 1);
        for (int it = 0; it < P.iters; it++) {
            double R[12], acc[29];
#pragma unroll
            for (int k = 0; k < 12; k++) R[k] = s_pose[k];
#pragma unroll
            for (int k = 0; k < 29; k++) acc[k] = 0.0;
            int sel = 0;
            for (int idx = threadIdx.x; idx < lv.n; idx += BLOCK) {
                const int j = idx / lv.nx, i = idx - j * lv.nx;
                const int x = lv.x_lo + 1 + i * lv.s, y = lv.y_lo + 1 + j * lv.s;
                const int d16 = P.disp16[(size_t)(y << L) * P.w0 + (x << L)];
                if (!((double)d16 >= P.d16_lo && (double)d16 <= P.d16_hi)) continue;
                const uint8_t* a = A + (size_t)y * lv.w + x;
                const int gx2 = (int)a[1] - (int)a[-1], gy2 = (int)a[lv.w] - (int)a[-lv.w];
                if (gx2 * gx2 + gy2 * gy2 < P.g2min) continue;
                sel++;
                const double d = (double)d16 / 16.0;
                const double W = P.q32 * d + P.q33;
                const double X = ((double)(x << L) + P.q03) / W, Y = ((double)(y << L) + P.q13) / W, Z = P.q23 / W;
                const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[3];
                const double yc = ((R[4] * X + R[5] * Y) + R[6] * Z) + R[7];
                const double zc = ((R[8] * X + R[9] * Y) + R[10] * Z) + R[11];
                if (!(zc > P.z_min)) continue;
                const double u = (lv.fx * xc) / zc + lv.cx, v = (lv.fy * yc) / zc + lv.cy;
                if (!(u >= xlo && u < xhi1 && v >= ylo && v < yhi1)) continue;       // (false for a NaN: nothing is read for it)
                const double fu = floor(u), fv = floor(v);
                const double ax = u - fu, ay = v - fv;
                const uint8_t* b = B + (size_t)(int)fv * lv.w + (int)fu;
                const double b00 = (double)b[0], b01 = (double)b[1], b10 = (double)b[lv.w], b11 = (double)b[lv.w + 1];
                const double Ib = (b00 * (1.0 - ax) + b01 * ax) * (1.0 - ay) + (b10 * (1.0 - ax) + b11 * ax) * ay;
                const double r = Ib - (double)a[0];
                const double ar = fabs(r);
                const double wt = ar <= P.huber ? 1.0 : P.huber / ar;
                const double gfx = (0.5 * (double)gx2) * lv.fx, gfy = (0.5 * (double)gy2) * lv.fy;
                const double a0 = gfx / zc, a1 = gfy / zc, a2 = -((gfx * xc + gfy * yc) / (zc * zc));
                const double jv[6] = { yc * a2 - zc * a1, zc * a0 - xc * a2, xc * a1 - yc * a0, a0, a1, a2 };
                double wj[6];
#pragma unroll
                for (int p = 0; p < 6; p++) wj[p] = wt * jv[p];
#pragma unroll
                for (int p = 0, k = 0; p < 6; p++)
#pragma unroll
                    for (int q = p; q < 6; q++, k++) acc[k] += wj[p] * jv[q];
#pragma unroll
                for (int p = 0; p < 6; p++) acc[21 + p] += wj[p] * r;
                acc[27] += 1.0;
                acc[28] += (wt * r) * r;
            }
#pragma unroll
            for (int k = 0; k < 29; k++) {
                const double sum = wave_sum_f64_dpp(acc[k]);
                if (lane == 0) s_red[wv][k] = sum;
            }
            for (int o = 32; o > 0; o >>= 1) sel += __shfl_xor(sel, o, 64);
            if (lane == 0) s_sel[wv] = sel;
            __syncthreads();
            if (threadIdx.x < 29) {                 // the waves' values in wave order, one sum per thread
                double sum = s_red[0][threadIdx.x];
#pragma unroll
                for (int q = 1; q < NW; q++) sum += s_red[q][threadIdx.x];
                s_sum[threadIdx.x] = sum;
            }
            __syncthreads();
            if (threadIdx.x == 0) direct_step(s_sum, s_sel, NW, it == 0, P.min_pixels, s_pose, s_last, &s_lv[L], &s_status, &s_done);
            __syncthreads();
            if (s_status != 0) { stop = true; break; }
        }
    }
    if (threadIdx.x == 0) {
        rec->status = s_status; rec->iters_done = s_done; rec->levels = P.levels; rec->pad = 0;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) rec->lv[l] = s_lv[l];
        for (int k = 0; k < 12; k++) rec->Rt[k] = s_pose[k];
        for (int k = 0; k < 27; k++) rec->sums[k] = s_last[k];
        rec->count = s_last[27]; rec->wr2 = s_last[28];
    }
}

// ---- the affine brightness form (include/vo355.h, vo_direct_align_ab; tests/direct_ab_ref.py restates it) -------------------------------
//   k_direct_align_ab  a sibling of k_direct_align with the same ownership, loops, reads and sum order; the state carries the gain k
//                      and the offset m of image B beside the pose (LDS, thread 0 commits all three together), the residual is
//                      (k I_b + m) - A, and an iteration is HELD (it < 2: the 29 sums of the six pose unknowns) or FREE (the 46 sums
//                      of eight unknowns: j[6] = I_b, j[7] = 1).  `it` is the same in every thread, so the branch between the two
//                      accumulation loops is uniform; a held iteration touches 29 accumulators, a free one 46.
template <int NU> struct DirectAbN { static constexpr int NH = NU * (NU + 1) / 2, NS = NH + NU + 2; };
#define VO_DIRECT_AB_NS 46

// One thread's part of an iteration with NU unknowns, then the wave's: the NS sums of wave wv into red[wv], its selected count into sel.
template <int BLOCK, int NU>
__device__ __forceinline__ void direct_ab_sums(const DirectPrm& P, const DirectLevel& lv, int L, const double* __restrict__ pose, double bk, double bm,
                                               double (*red)[VO_DIRECT_AB_NS], int* s_sel)
{
    constexpr int NH = DirectAbN<NU>::NH, NS = DirectAbN<NU>::NS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t* __restrict__ A = lv.A;
    const uint8_t* __restrict__ B = lv.B;
    const double xlo = (double)lv.x_lo, xhi1 = (double)(lv.x_hi - 1), ylo = (double)lv.y_lo, yhi1 = (double)(lv.y_hi - 1);
    double R[12], acc[NS];
#pragma unroll
    for (int k = 0; k < 12; k++) R[k] = pose[k];
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = 0.0;
    int sel = 0;
    for (int idx = threadIdx.x; idx < lv.n; idx += BLOCK) {
        const int j = idx / lv.nx, i = idx - j * lv.nx;
        const int x = lv.x_lo + 1 + i * lv.s, y = lv.y_lo + 1 + j * lv.s;
        const int d16 = P.disp16[(size_t)(y << L) * P.w0 + (x << L)];
        if (!((double)d16 >= P.d16_lo && (double)d16 <= P.d16_hi)) continue;
        const uint8_t* a = A + (size_t)y * lv.w + x;
        const int gx2 = (int)a[1] - (int)a[-1], gy2 = (int)a[lv.w] - (int)a[-lv.w];
        if (gx2 * gx2 + gy2 * gy2 < P.g2min) continue;
        sel++;
        const double d = (double)d16 / 16.0;
        const double W = P.q32 * d + P.q33;
        const double X = ((double)(x << L) + P.q03) / W, Y = ((double)(y << L) + P.q13) / W, Z = P.q23 / W;
        const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[3];
        const double yc = ((R[4] * X + R[5] * Y) + R[6] * Z) + R[7];
        const double zc = ((R[8] * X + R[9] * Y) + R[10] * Z) + R[11];
        if (!(zc > P.z_min)) continue;
        const double u = (lv.fx * xc) / zc + lv.cx, v = (lv.fy * yc) / zc + lv.cy;
        if (!(u >= xlo && u < xhi1 && v >= ylo && v < yhi1)) continue;       // (false for a NaN: nothing is read for it)
        const double fu = floor(u), fv = floor(v);
        const double ax = u - fu, ay = v - fv;
        const uint8_t* b = B + (size_t)(int)fv * lv.w + (int)fu;
        const double b00 = (double)b[0], b01 = (double)b[1], b10 = (double)b[lv.w], b11 = (double)b[lv.w + 1];
        const double Ib = (b00 * (1.0 - ax) + b01 * ax) * (1.0 - ay) + (b10 * (1.0 - ax) + b11 * ax) * ay;
        const double r = (bk * Ib + bm) - (double)a[0];
        const double ar = fabs(r);
        const double wt = ar <= P.huber ? 1.0 : P.huber / ar;
        const double gfx = (0.5 * (double)gx2) * lv.fx, gfy = (0.5 * (double)gy2) * lv.fy;
        const double a0 = gfx / zc, a1 = gfy / zc, a2 = -((gfx * xc + gfy * yc) / (zc * zc));
        double jv[NU];
        jv[0] = yc * a2 - zc * a1; jv[1] = zc * a0 - xc * a2; jv[2] = xc * a1 - yc * a0; jv[3] = a0; jv[4] = a1; jv[5] = a2;
        if constexpr (NU == 8) { jv[6] = Ib; jv[7] = 1.0; }
        double wj[NU];
#pragma unroll
        for (int p = 0; p < NU; p++) wj[p] = wt * jv[p];
#pragma unroll
        for (int p = 0, k = 0; p < NU; p++)
#pragma unroll
            for (int q = p; q < NU; q++, k++) acc[k] += wj[p] * jv[q];
#pragma unroll
        for (int p = 0; p < NU; p++) acc[NH + p] += wj[p] * r;
        acc[NH + NU] += 1.0;
        acc[NH + NU + 1] += (wt * r) * r;
    }
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const double sum = wave_sum_f64_dpp(acc[k]);
        if (lane == 0) red[wv][k] = sum;
    }
    for (int o = 32; o > 0; o >>= 1) sel += __shfl_xor(sel, o, 64);
    if (lane == 0) s_sel[wv] = sel;
}

// The end of an iteration with NU unknowns in one lane, as direct_step: S = the NS sums of the block.  The new pose, k and m are
// committed together or not at all; km = {k, m}; last = the sums of the last completed linearisation, *unknowns its size.
template <int NU>
__device__ __noinline__ void direct_ab_step(const double* S, const int* sel, int nw, bool first, int min_pixels, double* pose, double* km, double* last,
                                            int* unknowns, vo_direct_level* lv, int* status, int* done)
{
    constexpr int NH = DirectAbN<NU>::NH, NS = DirectAbN<NU>::NS;
    const int n = (int)S[NH + NU];
    if (first) {
        int nsel = 0;
        for (int q = 0; q < nw; q++) nsel += sel[q];
        lv->selected = nsel; lv->n_first = n; lv->wr2_first = S[NH + NU + 1];
    }
    lv->n_last = n; lv->wr2_last = S[NH + NU + 1];
    if (n < min_pixels) { *status = 2; return; }
    double H[NH], g[NU], d[NU];
#pragma unroll
    for (int k = 0; k < NU; k++) d[k] = 0.0;
    bool ok = isfinite(S[NH + NU + 1]);
#pragma unroll
    for (int k = 0; k < NH; k++) { H[k] = S[k]; ok = ok && isfinite(H[k]); }
#pragma unroll
    for (int k = 0; k < NU; k++) { g[k] = S[NH + k]; ok = ok && isfinite(g[k]); }
    ok = ok && pn_solve<NU>(H, g, d);
    double Rn[12], kn = km[0], mn = km[1];
#pragma unroll
    for (int k = 0; k < 12; k++) Rn[k] = pose[k];
    if (ok) {
        pn_apply_twist(Rn, d);
        if constexpr (NU == 8) { kn = kn + d[6]; mn = mn + d[7]; }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) ok = ok && isfinite(Rn[k]);
    ok = ok && isfinite(kn) && isfinite(mn) && kn > 0.0;
    if (!ok) { *status = -1; return; }
#pragma unroll
    for (int k = 0; k < 12; k++) pose[k] = Rn[k];
    km[0] = kn; km[1] = mn;
    for (int k = 0; k < NS; k++) last[k] = S[k];
    *unknowns = NU;
    *done = *done + 1;
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_direct_align_ab(DirectPrm P, vo_direct_ab_rec* __restrict__ rec)
{
    constexpr int NW = BLOCK / 64, NS = VO_DIRECT_AB_NS;
    static_assert(DirectAbN<8>::NS == NS && DirectAbN<6>::NS == 29, "the sums of a free and of a held iteration");
    __shared__ double s_red[NW][NS], s_sum[NS], s_pose[12], s_km[2], s_last[NS];
    __shared__ int s_sel[NW], s_status, s_done, s_unknowns;
    __shared__ vo_direct_level s_lv[VO_DIRECT_MAX_LEVELS];
    if (threadIdx.x == 0) {
        for (int k = 0; k < 12; k++) s_pose[k] = P.Rt0[k];
        for (int k = 0; k < NS; k++) s_last[k] = 0.0;
        s_km[0] = 1.0; s_km[1] = 0.0;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) {
            s_lv[l].s = l < P.levels ? P.lv[l].s : 0;
            s_lv[l].selected = s_lv[l].n_first = s_lv[l].n_last = 0;
            s_lv[l].wr2_first = s_lv[l].wr2_last = 0.0;
        }
        s_status = 0; s_done = 0; s_unknowns = 6;
    }
    __syncthreads();
    bool stop = false;
    for (int L = P.levels - 1; L >= 0 && !stop; --L) {
        const DirectLevel lv = P.lv[L];
        for (int it = 0; it < P.iters; it++) {
            const bool held = it < 2;                  // (the same in every thread)
            const int ns = held ? DirectAbN<6>::NS : NS;
            if (held) direct_ab_sums<BLOCK, 6>(P, lv, L, s_pose, s_km[0], s_km[1], s_red, s_sel);
            else direct_ab_sums<BLOCK, 8>(P, lv, L, s_pose, s_km[0], s_km[1], s_red, s_sel);
            __syncthreads();
            if ((int)threadIdx.x < ns) {               // the waves' values in wave order, one sum per thread
                double sum = s_red[0][threadIdx.x];
#pragma unroll
                for (int q = 1; q < NW; q++) sum += s_red[q][threadIdx.x];
                s_sum[threadIdx.x] = sum;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                if (held) direct_ab_step<6>(s_sum, s_sel, NW, it == 0, P.min_pixels, s_pose, s_km, s_last, &s_unknowns, &s_lv[L], &s_status, &s_done);
                else direct_ab_step<8>(s_sum, s_sel, NW, it == 0, P.min_pixels, s_pose, s_km, s_last, &s_unknowns, &s_lv[L], &s_status, &s_done);
            }
            __syncthreads();
            if (s_status != 0) { stop = true; break; }
        }
    }
    if (threadIdx.x == 0) {
        const int nu = s_unknowns, nh = nu * (nu + 1) / 2;
        rec->status = s_status; rec->iters_done = s_done; rec->levels = P.levels; rec->unknowns = nu;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) rec->lv[l] = s_lv[l];
        for (int k = 0; k < 12; k++) rec->Rt[k] = s_pose[k];
        rec->k = s_km[0]; rec->m = s_km[1];
        for (int k = 0; k < 44; k++) rec->sums[k] = k < nh + nu ? s_last[k] : 0.0;
        rec->count = s_last[nh + nu]; rec->wr2 = s_last[nh + nu + 1];
    }
}

// ---- the keypoint-patch form (include/vo355.h, vo_direct_align_kp; tests/direct_kp_ref.py restates it) ---------------------------------
//   k_direct_align_kp  a sibling of k_direct_align: the same workgroup, sums, sum order, barriers and direct_step; the POINTS are the
//                      patch pixels of slot a's depth-carrying keypoints instead of a lattice on the disparity.  Thread t owns the point
//                      indices idx = t modulo the block size, ascending, over n patch^2 (idx = i patch^2 + (dy + hp) patch + (dx + hp));
//                      the keypoint's position and depth are re-read per point (three float loads that hit the cache: nothing is
//                      packed, no scratch memory).  A position or depth that is not finite, not positive or outside the image is
//                      refused in floating point BEFORE the conversion to an integer, and a keypoint is in use at a level only when
//                      its patch and the ring the gradient reads lie in the level rectangle: every read of A is inside it by that
//                      test, every read of B by the test on (u, v), as in k_direct_align.  The keypoints in use are counted in the
//                      first iteration of a level (at the first pixel of each patch) and summed like the selected counts.
//                      The uniform float64 parameters (huber, z_min, three entries of Q, the level intrinsics) are written to LDS by
//                      thread 0 and read back by every thread: taken from the kernel arguments they sit in scalar registers, and
//                      with the keypoint pointers, the patch geometry and the crop origin beside k_direct_align's set the scalar
//                      file overflowed (15 spilled to lanes); from LDS they live in vector registers, of which there are enough.
struct DirectKpPrm {
    DirectLevel lv[VO_DIRECT_MAX_LEVELS];   // (s, nx, n are not read)
    const float *kp_xy, *kp_xyz;            // slot a: crop pixels (n, 2) and points (n, 3)
    int n, patch, w0, h0, levels, iters, min_pixels, g2min;
    float ox, oy;                           // the crop origin
    double huber, z_min, q03, q13, q23;
    double Rt0[12];
};

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_direct_align_kp(DirectKpPrm P, vo_direct_rec* __restrict__ rec)
{
    constexpr int NW = BLOCK / 64;
    __shared__ double s_red[NW][29], s_sum[29], s_pose[12], s_last[29];
    __shared__ double s_c[5], s_k[VO_DIRECT_MAX_LEVELS][4];     // the uniform float64 parameters: read back into vector registers
    __shared__ int s_sel[NW], s_kps[NW], s_status, s_done;
    __shared__ vo_direct_level s_lv[VO_DIRECT_MAX_LEVELS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        for (int k = 0; k < 12; k++) s_pose[k] = P.Rt0[k];
        for (int k = 0; k < 29; k++) s_last[k] = 0.0;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) {
            s_lv[l].s = s_lv[l].selected = s_lv[l].n_first = s_lv[l].n_last = 0;
            s_lv[l].wr2_first = s_lv[l].wr2_last = 0.0;
        }
        s_status = 0; s_done = 0;
        s_c[0] = P.huber; s_c[1] = P.z_min; s_c[2] = P.q03; s_c[3] = P.q13; s_c[4] = P.q23;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) { s_k[l][0] = P.lv[l].fx; s_k[l][1] = P.lv[l].fy; s_k[l][2] = P.lv[l].cx; s_k[l][3] = P.lv[l].cy; }
    }
    __syncthreads();
    const double huber = s_c[0], z_min = s_c[1], q03 = s_c[2], q13 = s_c[3], q23 = s_c[4];
    const unsigned patch = (unsigned)P.patch, pp = patch * patch, total = (unsigned)P.n * pp;      // (the host keeps n patch^2 below 2^31)
    const int hp = P.patch / 2;
    const float w0 = (float)P.w0, h0 = (float)P.h0;
    bool stop = false;
    for (int L = P.levels - 1; L >= 0 && !stop; --L) {
        const DirectLevel lv = P.lv[L];
        const uint8_t* __restrict__ A = lv.A;
        const uint8_t* __restrict__ B = lv.B;
        const double xlo = (double)lv.x_lo, xhi1 = (double)(lv.x_hi - 1), ylo = (double)lv.y_lo, yhi1 = (double)(lv.y_hi - 1);
        const double rl = 1.0 / (double)(1 << L);
        const double fxl = s_k[L][0], fyl = s_k[L][1], cxl = s_k[L][2], cyl = s_k[L][3];
        for (int it = 0; it < P.iters; it++) {
            double R[12], acc[29];
#pragma unroll
            for (int k = 0; k < 12; k++) R[k] = s_pose[k];
#pragma unroll
            for (int k = 0; k < 29; k++) acc[k] = 0.0;
            int sel = 0, kps = 0;
            for (unsigned idx = threadIdx.x; idx < total; idx += BLOCK) {
                const unsigned i = idx / pp, rem = idx - i * pp;
                const int pj = (int)(rem / patch), pi = (int)(rem - (unsigned)pj * patch);
                const float vxf = P.kp_xy[2 * (size_t)i] + P.ox, vyf = P.kp_xy[2 * (size_t)i + 1] + P.oy;
                const float zf = P.kp_xyz[3 * (size_t)i + 2];
                // (w and h are exact in float32, so these comparisons are the float64 ones; false for a NaN: never an index)
                if (!(isfinite(zf) && zf > 0.f && vxf >= 0.f && vxf < w0 && vyf >= 0.f && vyf < h0)) continue;
                const int cx = (int)rint((double)vxf * rl), cy = (int)rint((double)vyf * rl);    // (a power of two: the product is the quotient)
                if (!(cx - hp >= lv.x_lo + 1 && cx + hp <= lv.x_hi - 2 && cy - hp >= lv.y_lo + 1 && cy + hp <= lv.y_hi - 2)) continue;
                if (rem == 0) kps++;
                const int x = cx + pi - hp, y = cy + pj - hp;
                const uint8_t* a = A + (size_t)y * lv.w + x;
                const int gx2 = (int)a[1] - (int)a[-1], gy2 = (int)a[lv.w] - (int)a[-lv.w];
                if (gx2 * gx2 + gy2 * gy2 < P.g2min) continue;
                sel++;
                const double Z = (double)zf;
                const double si = Z / q23;
                const double X = ((double)(x << L) + q03) * si, Y = ((double)(y << L) + q13) * si;
                const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[3];
                const double yc = ((R[4] * X + R[5] * Y) + R[6] * Z) + R[7];
                const double zc = ((R[8] * X + R[9] * Y) + R[10] * Z) + R[11];
                if (!(zc > z_min)) continue;
                const double u = (fxl * xc) / zc + cxl, v = (fyl * yc) / zc + cyl;
                if (!(u >= xlo && u < xhi1 && v >= ylo && v < yhi1)) continue;       // (false for a NaN: nothing is read for it)
                const double fu = floor(u), fv = floor(v);
                const double ax = u - fu, ay = v - fv;
                const uint8_t* b = B + (size_t)(int)fv * lv.w + (int)fu;
                const double b00 = (double)b[0], b01 = (double)b[1], b10 = (double)b[lv.w], b11 = (double)b[lv.w + 1];
                const double Ib = (b00 * (1.0 - ax) + b01 * ax) * (1.0 - ay) + (b10 * (1.0 - ax) + b11 * ax) * ay;
                const double r = Ib - (double)a[0];
                const double ar = fabs(r);
                const double wt = ar <= huber ? 1.0 : huber / ar;
                const double gfx = (0.5 * (double)gx2) * fxl, gfy = (0.5 * (double)gy2) * fyl;
                const double a0 = gfx / zc, a1 = gfy / zc, a2 = -((gfx * xc + gfy * yc) / (zc * zc));
                const double jv[6] = { yc * a2 - zc * a1, zc * a0 - xc * a2, xc * a1 - yc * a0, a0, a1, a2 };
                double wj[6];
#pragma unroll
                for (int p = 0; p < 6; p++) wj[p] = wt * jv[p];
#pragma unroll
                for (int p = 0, k = 0; p < 6; p++)
#pragma unroll
                    for (int q = p; q < 6; q++, k++) acc[k] += wj[p] * jv[q];
#pragma unroll
                for (int p = 0; p < 6; p++) acc[21 + p] += wj[p] * r;
                acc[27] += 1.0;
                acc[28] += (wt * r) * r;
            }
#pragma unroll
            for (int k = 0; k < 29; k++) {
                const double sum = wave_sum_f64_dpp(acc[k]);
                if (lane == 0) s_red[wv][k] = sum;
            }
            for (int o = 32; o > 0; o >>= 1) { sel += __shfl_xor(sel, o, 64); kps += __shfl_xor(kps, o, 64); }
            if (lane == 0) { s_sel[wv] = sel; s_kps[wv] = kps; }
            __syncthreads();
            if (threadIdx.x < 29) {                 // the waves' values in wave order, one sum per thread
                double sum = s_red[0][threadIdx.x];
#pragma unroll
                for (int q = 1; q < NW; q++) sum += s_red[q][threadIdx.x];
                s_sum[threadIdx.x] = sum;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                if (it == 0) {
                    int nk = 0;
                    for (int q = 0; q < NW; q++) nk += s_kps[q];
                    s_lv[L].s = nk;
                }
                direct_step(s_sum, s_sel, NW, it == 0, P.min_pixels, s_pose, s_last, &s_lv[L], &s_status, &s_done);
            }
            __syncthreads();
            if (s_status != 0) { stop = true; break; }
        }
    }
    if (threadIdx.x == 0) {
        rec->status = s_status; rec->iters_done = s_done; rec->levels = P.levels; rec->pad = P.patch;
        for (int l = 0; l < VO_DIRECT_MAX_LEVELS; l++) rec->lv[l] = s_lv[l];
        for (int k = 0; k < 12; k++) rec->Rt[k] = s_pose[k];
        for (int k = 0; k < 27; k++) rec->sums[k] = s_last[k];
        rec->count = s_last[27]; rec->wr2 = s_last[28];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static inline int direct_lattice_n(int lo, int hi, int s) { return hi - lo - 2 > 0 ? (hi - lo - 2 + s - 1) / s : 0; }

// Both entries: the checks, the pyramids, the parameters, the one launch (ab: k_direct_align_ab, whose iters start at 3) and the
// one synchronisation; rec_out is a vo_direct_rec or a vo_direct_ab_rec.
static int direct_align_run(vo_ctx* ctx, const char* who, bool ab, int slot_a, int slot_b, const double* K4v, const double* Rt0, int levels, int iters,
                            int max_points, int grad_min, double huber, double dmin, double dmax, double z_min, int min_pixels, void* rec_out)
{
    const int iters_lo = ab ? 3 : 1;
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !K4v || !Rt0 || !rec_out)
        return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (levels < 1 || levels > VO_DIRECT_MAX_LEVELS) return vo_fail(ctx, VO_E_ARG, "%s: levels %d (1 .. %d)", who, levels, VO_DIRECT_MAX_LEVELS);
    if (iters < iters_lo || iters > 20) return vo_fail(ctx, VO_E_ARG, "%s: iters %d (%d .. 20)", who, iters, iters_lo);
    if (max_points < 1) return vo_fail(ctx, VO_E_ARG, "%s: max_points %d (>= 1)", who, max_points);
    if (grad_min < 0 || grad_min > 255) return vo_fail(ctx, VO_E_ARG, "%s: grad_min %d (0 .. 255)", who, grad_min);
    if (min_pixels < 6) return vo_fail(ctx, VO_E_ARG, "%s: min_pixels %d (>= 6)", who, min_pixels);
    if (!(isfinite(huber) && huber > 0 && isfinite(dmin) && isfinite(dmax) && dmin > 0 && dmin <= dmax && isfinite(z_min) && z_min >= 0))
        return vo_fail(ctx, VO_E_ARG, "%s: huber > 0, 0 < dmin <= dmax and z_min >= 0, all finite", who);
    for (int k = 0; k < 12; k++)
        if (!isfinite(Rt0[k])) return vo_fail(ctx, VO_E_ARG, "%s: Rt0 is not finite", who);
    if (!(isfinite(K4v[0]) && isfinite(K4v[1]) && isfinite(K4v[2]) && isfinite(K4v[3]) && K4v[0] > 0 && K4v[1] > 0))
        return vo_fail(ctx, VO_E_ARG, "%s: K4 must be finite with fx, fy > 0", who);
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_pair || !b.has_pair) return vo_fail(ctx, VO_E_STATE, "%s: slots %d and %d must both hold a pair", who, slot_a, slot_b);
    if (slot_sparse(a)) return vo_fail(ctx, VO_E_STATE, "%s: slot %d is a sparse slot (its keypoints carry depth): no dense disparity", who, slot_a);
    if (!a.has_disp) return vo_fail(ctx, VO_E_STATE, "%s: slot %d holds no dense disparity", who, slot_a);
    if (a.w != b.w || a.h != b.h) return vo_fail(ctx, VO_E_STATE, "%s: the slots' images differ in shape (%dx%d, %dx%d)", who, a.w, a.h, b.w, b.h);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }

    DirectPrm P;
    memset(&P, 0, sizeof(P));
    const uint8_t *pa[VO_KLT_MAX_LEVELS], *pb[VO_KLT_MAX_LEVELS];
    int lw[VO_KLT_MAX_LEVELS], lh[VO_KLT_MAX_LEVELS];
    int rc = klt_ws_prepare(ctx);
    if (!rc) rc = klt_pyr_enqueue(ctx, a.left, b.left, a.w, a.h, levels, pa, pb, lw, lh);
    if (rc) return rc;
    int rx0 = 0, ry0 = 0, rx1 = a.w, ry1 = a.h;
    if (ctx->has_roi) {
        rx0 = ctx->roi[0] < a.w ? ctx->roi[0] : a.w; ry0 = ctx->roi[1] < a.h ? ctx->roi[1] : a.h;
        rx1 = ctx->roi[2] < a.w ? ctx->roi[2] : a.w; ry1 = ctx->roi[3] < a.h ? ctx->roi[3] : a.h;
    }
    for (int l = 0; l < levels; l++) {
        DirectLevel& v = P.lv[l];
        const int f = 1 << l;
        v.A = pa[l]; v.B = pb[l]; v.w = lw[l];
        if (ctx->has_roi) { v.x_lo = (rx0 + f - 1) / f; v.x_hi = rx1 > 0 ? rx1 / f : 0; v.y_lo = (ry0 + f - 1) / f; v.y_hi = ry1 > 0 ? ry1 / f : 0; }
        else { v.x_lo = 0; v.x_hi = lw[l]; v.y_lo = 0; v.y_hi = lh[l]; }
        int s = 1;
        while ((long long)direct_lattice_n(v.x_lo, v.x_hi, s) * direct_lattice_n(v.y_lo, v.y_hi, s) > max_points) s++;
        v.s = s; v.nx = direct_lattice_n(v.x_lo, v.x_hi, s);
        v.n = v.nx * direct_lattice_n(v.y_lo, v.y_hi, s);
        if (v.nx == 0) { v.nx = 1; v.n = 0; }
        v.fx = K4v[0] / (double)f; v.fy = K4v[1] / (double)f; v.cx = K4v[2] / (double)f; v.cy = K4v[3] / (double)f;
    }
    P.disp16 = a.disp16; P.w0 = a.w; P.levels = levels; P.iters = iters; P.min_pixels = min_pixels; P.g2min = 4 * grad_min * grad_min;
    P.d16_lo = 16.0 * dmin; P.d16_hi = 16.0 * dmax; P.huber = huber; P.z_min = z_min;
    P.q03 = ctx->Q[3]; P.q13 = ctx->Q[7]; P.q23 = ctx->Q[11]; P.q32 = ctx->Q[14]; P.q33 = ctx->Q[15];
    for (int k = 0; k < 12; k++) P.Rt0[k] = Rt0[k];
    const size_t rec_bytes = ab ? sizeof(vo_direct_ab_rec) : sizeof(vo_direct_rec);
    memset(ctx->pinned, 0, rec_bytes);
    {
        StageTimer t(ctx, VO_T_POSE);
        if (ab) hipLaunchKernelGGL(k_direct_align_ab<VO_DIRECT_BLOCK>, dim3(1), dim3(VO_DIRECT_BLOCK), 0, ctx->stream, P, (vo_direct_ab_rec*)ctx->pinned);
        else hipLaunchKernelGGL(k_direct_align<VO_DIRECT_BLOCK>, dim3(1), dim3(VO_DIRECT_BLOCK), 0, ctx->stream, P, (vo_direct_rec*)ctx->pinned);
        VO_CHECK_LAUNCH(ctx);
    }
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    if ((rc = slot_health(ctx, a, slot_a))) return rc;       // never a pose from an undefined disparity (b's is not read)
    memcpy(rec_out, ctx->pinned, rec_bytes);
    return VO_OK;
}

extern "C" int vo_direct_align(vo_ctx* ctx, int slot_a, int slot_b, const double* K4v, const double* Rt0, int levels, int iters, int max_points,
                               int grad_min, double huber, double dmin, double dmax, double z_min, int min_pixels, vo_direct_rec* rec_out)
{
    return direct_align_run(ctx, "vo_direct_align", false, slot_a, slot_b, K4v, Rt0, levels, iters, max_points, grad_min, huber, dmin, dmax, z_min,
                            min_pixels, rec_out);
}

// The keypoint-patch entry: vo_direct_align's checks without the lattice and the disparity range, the same pyramids, rectangles and
// level intrinsics, the one launch (k_direct_align_kp) and the one synchronisation.
extern "C" int vo_direct_align_kp(vo_ctx* ctx, int slot_a, int slot_b, const double* K4v, const double* Rt0, int levels, int iters, int patch,
                                  int grad_min, double huber, double z_min, int min_pixels, vo_direct_rec* rec_out)
{
    const char* who = "vo_direct_align_kp";
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !K4v || !Rt0 || !rec_out)
        return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (levels < 1 || levels > VO_DIRECT_MAX_LEVELS) return vo_fail(ctx, VO_E_ARG, "%s: levels %d (1 .. %d)", who, levels, VO_DIRECT_MAX_LEVELS);
    if (iters < 1 || iters > 20) return vo_fail(ctx, VO_E_ARG, "%s: iters %d (1 .. 20)", who, iters);
    if (patch != 3 && patch != 5 && patch != 7) return vo_fail(ctx, VO_E_ARG, "%s: patch %d (3, 5 or 7)", who, patch);
    if (grad_min < 0 || grad_min > 255) return vo_fail(ctx, VO_E_ARG, "%s: grad_min %d (0 .. 255)", who, grad_min);
    if (min_pixels < 6) return vo_fail(ctx, VO_E_ARG, "%s: min_pixels %d (>= 6)", who, min_pixels);
    if (!(isfinite(huber) && huber > 0 && isfinite(z_min) && z_min >= 0)) return vo_fail(ctx, VO_E_ARG, "%s: huber > 0 and z_min >= 0, both finite", who);
    for (int k = 0; k < 12; k++)
        if (!isfinite(Rt0[k])) return vo_fail(ctx, VO_E_ARG, "%s: Rt0 is not finite", who);
    if (!(isfinite(K4v[0]) && isfinite(K4v[1]) && isfinite(K4v[2]) && isfinite(K4v[3]) && K4v[0] > 0 && K4v[1] > 0))
        return vo_fail(ctx, VO_E_ARG, "%s: K4 must be finite with fx, fy > 0", who);
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_pair || !b.has_pair) return vo_fail(ctx, VO_E_STATE, "%s: slots %d and %d must both hold a pair", who, slot_a, slot_b);
    if (!slot_sparse(a)) return vo_fail(ctx, VO_E_STATE, "%s: slot %d: the keypoints carry no depth (vo_sparse_stereo)", who, slot_a);
    if (a.w != b.w || a.h != b.h) return vo_fail(ctx, VO_E_STATE, "%s: the slots' images differ in shape (%dx%d, %dx%d)", who, a.w, a.h, b.w, b.h);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    if (!(isfinite(ctx->Q[11]) && ctx->Q[11] != 0.0)) return vo_fail(ctx, VO_E_STATE, "%s: Q[2][3] must be finite and not zero", who);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    if (a.n_kp < 0 || a.n_kp > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "%s: %d keypoints exceed capacity %d", who, a.n_kp, ctx->kp_cap);
    if ((long long)a.n_kp * patch * patch > 0x7fffffffLL) return vo_fail(ctx, VO_E_CAP, "%s: %d keypoints of %d x %d pixels exceed the index range", who, a.n_kp, patch, patch);

    DirectKpPrm P;
    memset(&P, 0, sizeof(P));
    const uint8_t *pa[VO_KLT_MAX_LEVELS], *pb[VO_KLT_MAX_LEVELS];
    int lw[VO_KLT_MAX_LEVELS], lh[VO_KLT_MAX_LEVELS];
    int rc = klt_ws_prepare(ctx);
    if (!rc) rc = klt_pyr_enqueue(ctx, a.left, b.left, a.w, a.h, levels, pa, pb, lw, lh);
    if (rc) return rc;
    int rx0 = 0, ry0 = 0, rx1 = a.w, ry1 = a.h;
    if (ctx->has_roi) {
        rx0 = ctx->roi[0] < a.w ? ctx->roi[0] : a.w; ry0 = ctx->roi[1] < a.h ? ctx->roi[1] : a.h;
        rx1 = ctx->roi[2] < a.w ? ctx->roi[2] : a.w; ry1 = ctx->roi[3] < a.h ? ctx->roi[3] : a.h;
    }
    for (int l = 0; l < levels; l++) {
        DirectLevel& v = P.lv[l];
        const int f = 1 << l;
        v.A = pa[l]; v.B = pb[l]; v.w = lw[l];
        if (ctx->has_roi) { v.x_lo = (rx0 + f - 1) / f; v.x_hi = rx1 > 0 ? rx1 / f : 0; v.y_lo = (ry0 + f - 1) / f; v.y_hi = ry1 > 0 ? ry1 / f : 0; }
        else { v.x_lo = 0; v.x_hi = lw[l]; v.y_lo = 0; v.y_hi = lh[l]; }
        v.fx = K4v[0] / (double)f; v.fy = K4v[1] / (double)f; v.cx = K4v[2] / (double)f; v.cy = K4v[3] / (double)f;
    }
    P.kp_xy = a.kp_xy; P.kp_xyz = a.kp_xyz; P.n = a.n_kp; P.patch = patch; P.w0 = a.w; P.h0 = a.h;
    P.levels = levels; P.iters = iters; P.min_pixels = min_pixels; P.g2min = 4 * grad_min * grad_min;
    P.ox = ctx->has_roi ? (float)ctx->roi[0] : 0.f; P.oy = ctx->has_roi ? (float)ctx->roi[1] : 0.f;
    P.huber = huber; P.z_min = z_min; P.q03 = ctx->Q[3]; P.q13 = ctx->Q[7]; P.q23 = ctx->Q[11];
    for (int k = 0; k < 12; k++) P.Rt0[k] = Rt0[k];
    memset(ctx->pinned, 0, sizeof(vo_direct_rec));
    {
        StageTimer t(ctx, VO_T_POSE);
        hipLaunchKernelGGL(k_direct_align_kp<VO_DIRECT_BLOCK>, dim3(1), dim3(VO_DIRECT_BLOCK), 0, ctx->stream, P, (vo_direct_rec*)ctx->pinned);
        VO_CHECK_LAUNCH(ctx);
    }
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    memcpy(rec_out, ctx->pinned, sizeof(vo_direct_rec));
    return VO_OK;
}

extern "C" int vo_direct_align_ab(vo_ctx* ctx, int slot_a, int slot_b, const double* K4v, const double* Rt0, int levels, int iters, int max_points,
                                  int grad_min, double huber, double dmin, double dmax, double z_min, int min_pixels, vo_direct_ab_rec* rec_out)
{
    return direct_align_run(ctx, "vo_direct_align_ab", true, slot_a, slot_b, K4v, Rt0, levels, iters, max_points, grad_min, huber, dmin, dmax, z_min,
                            min_pixels, rec_out);
}
