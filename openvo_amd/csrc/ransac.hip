// RANSAC essential-matrix hypothesis generation + Sampson inlier scoring on gfx950
// (BASELINE config 5: monocular 1920x1080, 8000 keypoints, 5000 hypotheses).
//
// The reference has NO RANSAC (its pose is a closed-form Umeyama fit): this stage has
// no openVO counterpart and is defined by this build; the CPU restatement lives with the other
// test infrastructure and the two must agree bit for bit (hypothesis order, inlier counts, masks).
//
//   k_ransac_hyp    one lane per hypothesis: counter-based hash sampling of 8 distinct matches,
//                   A^T A (9x9) in float64, cyclic Jacobi for the smallest eigenvector, 3x3 SVD
//                   projection on the essential manifold, F = K^-T E K^-1 rounded to float32
//   k_ransac_score  one wave per hypothesis (4 per block); lanes stride over the matches held in
//                   LDS-free registers, Sampson test in float32 with a fixed operation order, inlier
//                   count by __ballot + popcount -- 40 M residuals at config 5
//   k_ransac_best   argmax (ties -> lowest hypothesis) with a DPP-free shuffle reduction, then the
//                   winner's inlier mask
// What every step shares is written once: rs_sample_distinct (the sampler of all three generators), rs_block_argmax (the winner
// rule), rs_score_wave / rs_winner_model / rs_inlier_of over a model trait (SampsonModel, ReprojModel), pnp_project, and the
// workspace layouts of ransac_ws.h.
#include <math.h>
#include "vo_internal.h"

__device__ __forceinline__ uint32_t lowbias32(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}

// N distinct indices in [0, n) for hypothesis h by counter-based hash draws: a draw that repeats an earlier index is drawn
// again, and the 65th attempt is kept whatever it is (n < N cannot loop for ever)
template <int N>
__device__ __forceinline__ void rs_sample_distinct(uint32_t seed, int h, int n, int* idx)
{
    for (int j = 0; j < N; j++) {
        uint32_t attempt = 0;
        for (;;) {
            uint32_t r = lowbias32(seed ^ lowbias32((uint32_t)h * 0x9E3779B9u + (uint32_t)j * 0x85EBCA6Bu + attempt * 0xC2B2AE35u));
            int cand = (int)(r % (uint32_t)n), dup = 0;
            for (int k = 0; k < j; k++) dup |= idx[k] == cand;
            if (!dup || attempt >= 64) { idx[j] = cand; break; }
            attempt++;
        }
    }
}

// The winner rule, spelled out here alone: the hypothesis with the most inliers, the lowest index among equals.  For one block
// of 1 .. 16 whole waves; s_key: one word of LDS per wave.  Ends behind a barrier: every thread holds the winner and its count.
__device__ __forceinline__ void rs_block_argmax(const int32_t* __restrict__ counts, int iters, long long* s_key, int& best, int& best_count)
{
    long long key = -1;
    for (int h = threadIdx.x; h < iters; h += blockDim.x) {
        const long long k = ((long long)counts[h] << 32) | (long long)(0x7fffffff - h);
        key = k > key ? k : key;
    }
    for (int o = 32; o > 0; o >>= 1) { const long long other = __shfl_xor(key, o, 64); key = other > key ? other : key; }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < (int)(blockDim.x >> 6); q++) key = s_key[q] > key ? s_key[q] : key;
        s_key[0] = key;
    }
    __syncthreads();
    key = s_key[0];
    best = 0x7fffffff - (int)(key & 0x7fffffffLL);
    best_count = (int)(key >> 32);
}

__device__ void rs_cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// one-sided Jacobi SVD of a 3x3 matrix (same algorithm as the pose path)
__device__ void rs_svd3(const double* A, double* U, double* w, double* Vt)
{
    double G[9], V[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    for (int k = 0; k < 9; k++) G[k] = A[k];
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; i++) {
                    al += G[i * 3 + p] * G[i * 3 + p];
                    be += G[i * 3 + q] * G[i * 3 + q];
                    ga += G[i * 3 + p] * G[i * 3 + q];
                }
                if (fabs(ga) <= 1e-300 || fabs(ga) <= 2.2204460492503131e-16 * sqrt(al * be)) continue;
                rotated = true;
                double zeta = (be - al) / (2.0 * ga);
                double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; i++) {
                    double gp = G[i * 3 + p], gq = G[i * 3 + q];
                    G[i * 3 + p] = c * gp - s * gq;
                    G[i * 3 + q] = s * gp + c * gq;
                    double vp = V[i * 3 + p], vq = V[i * 3 + q];
                    V[i * 3 + p] = c * vp - s * vq;
                    V[i * 3 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    // (the order of the singular values is kept in three scalars and applied through selects: an index array read with a
    // run-time index would put G, V and sv into scratch memory)
    double sv[3];
    for (int j = 0; j < 3; j++) sv[j] = sqrt(G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j]);
#define RS_SEL3(a, b, c, o) ((o) == 0 ? (a) : (o) == 1 ? (b) : (c))
#define RS_SV(o) RS_SEL3(sv[0], sv[1], sv[2], o)
    int o0 = 0, o1 = 1, o2 = 2;
    if (RS_SV(o1) > RS_SV(o0)) { const int t = o0; o0 = o1; o1 = t; }
    if (RS_SV(o2) > RS_SV(o0)) { const int t = o0; o0 = o2; o2 = t; }
    if (RS_SV(o2) > RS_SV(o1)) { const int t = o1; o1 = o2; o2 = t; }
    double Uc[3][3], Vc[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int o = j == 0 ? o0 : j == 1 ? o1 : o2;
        const double so = RS_SV(o);
        w[j] = so;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            Vc[j][i] = RS_SEL3(V[i * 3], V[i * 3 + 1], V[i * 3 + 2], o);
            Uc[j][i] = so > 0 ? RS_SEL3(G[i * 3], G[i * 3 + 1], G[i * 3 + 2], o) / so : 0.0;
        }
    }
#undef RS_SV
#undef RS_SEL3
    const double tiny = w[0] * 1e-300 + 1e-300;
    if (w[1] <= tiny) {
        double a[3] = { 1, 0, 0 };
        if (fabs(Uc[0][0]) > 0.9) { a[0] = 0; a[1] = 1; }
        rs_cross3(Uc[0], a, Uc[1]);
        double nn = sqrt(Uc[1][0] * Uc[1][0] + Uc[1][1] * Uc[1][1] + Uc[1][2] * Uc[1][2]);
        for (int i = 0; i < 3; i++) Uc[1][i] /= nn;
    }
    if (w[2] <= tiny || w[2] <= 1e-14 * w[0]) {
        rs_cross3(Uc[0], Uc[1], Uc[2]);
        double nn = sqrt(Uc[2][0] * Uc[2][0] + Uc[2][1] * Uc[2][1] + Uc[2][2] * Uc[2][2]);
        if (nn > 0) for (int i = 0; i < 3; i++) Uc[2][i] /= nn;
    }
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) { U[i * 3 + j] = Uc[j][i]; Vt[j * 3 + i] = Vc[j][i]; }
}

struct K4 { double fx, fy, cx, cy; };

// n_dev (may be NULL): the number of correspondences when only the device knows it (vo_mono_pair: the ratio test's
// survivor count); fewer than 8 correspondences give all-zero hypotheses that score no inlier
// F = K^-T E K^-1, scaled to max |entry| = 1, rounded to float32
__device__ void rs_emit(const double* E, const K4& K, int h, double* __restrict__ E_out, float* __restrict__ F_out)
{
    const double ifx = 1.0 / K.fx, ify = 1.0 / K.fy;
    const double Ki[9] = { ifx, 0, -K.cx * ifx, 0, ify, -K.cy * ify, 0, 0, 1 };
    double T[9], Fd[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += E[r * 3 + k] * Ki[k * 3 + c]; T[r * 3 + c] = s; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += Ki[k * 3 + r] * T[k * 3 + c]; Fd[r * 3 + c] = s; }
    double mx = 0;
    for (int k = 0; k < 9; k++) if (fabs(Fd[k]) > mx) mx = fabs(Fd[k]);
    const double sc = mx > 0 ? 1.0 / mx : 1.0;
    for (int k = 0; k < 9; k++) { E_out[(size_t)h * 9 + k] = E[k]; F_out[(size_t)h * 9 + k] = (float)(Fd[k] * sc); }
}

__global__ void __launch_bounds__(64) k_ransac_hyp(const float* __restrict__ p1, const float* __restrict__ p2, int n, K4 K,
                                                   int iters, uint32_t seed, double* __restrict__ E_out, float* __restrict__ F_out,
                                                   const int* __restrict__ n_dev)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= iters) return;
    if (n_dev) n = *n_dev;
    if (n < 8) {
        for (int k = 0; k < 9; k++) { E_out[(size_t)h * 9 + k] = 0.0; F_out[(size_t)h * 9 + k] = 0.f; }
        return;
    }
    int idx[8];
    rs_sample_distinct<8>(seed, h, n, idx);
    double a[9][9];
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) a[i][j] = 0.0;
    for (int s = 0; s < 8; s++) {
        const int i = idx[s];
        const double x1 = ((double)p1[2 * i] - K.cx) / K.fx, y1 = ((double)p1[2 * i + 1] - K.cy) / K.fy;
        const double x2 = ((double)p2[2 * i] - K.cx) / K.fx, y2 = ((double)p2[2 * i + 1] - K.cy) / K.fy;
        const double r[9] = { x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0 };
        for (int u = 0; u < 9; u++) for (int v = 0; v < 9; v++) a[u][v] += r[u] * r[v];
    }
    double v[9][9];
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 9; p++) { diag += a[p][p] * a[p][p]; for (int q = p + 1; q < 9; q++) off += a[p][q] * a[p][q]; }
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 9; k++) { const double x = a[k][p], y = a[k][q]; a[k][p] = c * x - s * y; a[k][q] = s * x + c * y; }
                for (int k = 0; k < 9; k++) { const double x = a[p][k], y = a[q][k]; a[p][k] = c * x - s * y; a[q][k] = s * x + c * y; }
                for (int k = 0; k < 9; k++) { const double x = v[k][p], y = v[k][q]; v[k][p] = c * x - s * y; v[k][q] = s * x + c * y; }
            }
    }
    int m = 0;
    for (int i = 1; i < 9; i++) if (a[i][i] < a[m][m]) m = i;
    double e0[9], U[9], w[3], Vt[9], E[9];
    for (int k = 0; k < 9; k++) e0[k] = v[k][m];
    rs_svd3(e0, U, w, Vt);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) E[r * 3 + c] = U[r * 3 + 0] * Vt[0 * 3 + c] + U[r * 3 + 1] * Vt[1 * 3 + c];
    rs_emit(E, K, h, E_out, F_out);
}

#include "fivept.inc"

__device__ __forceinline__ bool sampson_inlier(const float* F, float u1, float v1, float u2, float v2, float thr2)
{
    const float fx0 = (F[0] * u1 + F[1] * v1) + F[2];
    const float fx1 = (F[3] * u1 + F[4] * v1) + F[5];
    const float fx2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float ft0 = (F[0] * u2 + F[3] * v2) + F[6];
    const float ft1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float num = (u2 * fx0 + v2 * fx1) + fx2;
    const float den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1;
    return (num * num) / den < thr2;
}

// A model trait names what the score and mask bodies below need of a model: W floats per hypothesis, the per-point test on the
// step's point arrays, and the live count -- fewer correspondences than a sample score nothing.
struct SampsonModel {                       // F (9 floats) on two streams of pixels
    static constexpr int W = 9;
    const float *p1, *p2;
    int min_n;                              // 8, or 6 for the five-point solver
    __device__ __forceinline__ int live(int n) const { return n < min_n ? 0 : n; }
    __device__ __forceinline__ bool inlier(const float* F, int i, float thr2) const
    {
        const float2 a = ((const float2*)p1)[i], b = ((const float2*)p2)[i];
        return sampson_inlier(F, a.x, a.y, b.x, b.y, thr2);
    }
};

template <class Model>
__device__ __forceinline__ void rs_winner_model(const float* __restrict__ M_all, int h, float* M)
{
#pragma unroll
    for (int k = 0; k < Model::W; k++) M[k] = M_all[(size_t)h * Model::W + k];
}

// point i under model M: an inlier only below the live count
template <class Model>
__device__ __forceinline__ bool rs_inlier_of(const Model& md, const float* M, int i, int live, float thr2)
{
    return i < live && md.inlier(M, i, thr2);
}

// one wave per hypothesis: lanes stride over the points, ballot + popcount.  n_dev (may be NULL): the count only the device knows
template <class Model>
__device__ __forceinline__ void rs_score_wave(const Model& md, int n, const float* __restrict__ M_all, int iters, float thr2,
                                              int32_t* __restrict__ counts, const int* __restrict__ n_dev)
{
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (h >= iters) return;
    if (n_dev) n = md.live(*n_dev);
    float M[Model::W];
    rs_winner_model<Model>(M_all, h, M);
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) cnt += __popcll(__ballot(rs_inlier_of(md, M, i0 + lane, n, thr2)));
    if (lane == 0) counts[h] = cnt;
}

// the winner's mask, one thread per point; with n_dev the points behind the live count are cleared
template <class Model>
__device__ __forceinline__ void rs_mask_point(const Model& md, int n, const float* __restrict__ M_all, const int32_t* __restrict__ best,
                                              float thr2, uint8_t* __restrict__ mask, const int* __restrict__ n_dev)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) { const int live = md.live(*n_dev); if (i < n && i >= live) mask[i] = 0; n = live; }
    if (i >= n) return;
    float M[Model::W];
    rs_winner_model<Model>(M_all, best[0], M);
    mask[i] = md.inlier(M, i, thr2) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_ransac_score(const float* __restrict__ p1, const float* __restrict__ p2, int n,
                                                     const float* __restrict__ F_all, int iters, float thr2, int32_t* __restrict__ counts,
                                                     const int* __restrict__ n_dev, int min_n)
{
    rs_score_wave(SampsonModel{ p1, p2, min_n }, n, F_all, iters, thr2, counts, n_dev);
}

__global__ void __launch_bounds__(1024) k_ransac_best(const int32_t* __restrict__ counts, int iters, int32_t* __restrict__ best /*[2]: index, count*/)
{
    __shared__ long long s_key[16];
    int b, c;
    rs_block_argmax(counts, iters, s_key, b, c);
    if (threadIdx.x == 0) { best[0] = b; best[1] = c; }
}

__global__ void k_ransac_mask(const float* __restrict__ p1, const float* __restrict__ p2, int n, const float* __restrict__ F_all,
                              const int32_t* __restrict__ best, float thr2, uint8_t* __restrict__ mask, const int* __restrict__ n_dev, int min_n)
{
    rs_mask_point(SampsonModel{ p1, p2, min_n }, n, F_all, best, thr2, mask, n_dev);
}

// the five-point kernel keeps its matrices in 100 KB of LDS per wave: above the 64 KB a launch may ask for by default
// (the attribute belongs to the device's copy of the code object; a context lives on one device and in one thread: set once each)
static int hyp5_prepare(vo_ctx* ctx)
{
    if (ctx->hyp5_ready) return VO_OK;
    VO_HIP(ctx, hipFuncSetAttribute((const void*)k_ransac_hyp5, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FP_LDS_DOUBLES * sizeof(double))));
    ctx->hyp5_ready = true;
    return VO_OK;
}

static int ransac_essential(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K4v, int iters, float thr,
                            uint32_t seed, double* E9_out, uint8_t* mask_out, int32_t* counts_out, int32_t* best2_out, int solver)
{
    const int min_n = solver == 5 ? 6 : 8;
    if (!ctx || !pts1 || !pts2 || !K4v || !E9_out || !best2_out) return vo_fail(ctx, VO_E_ARG, "vo_ransac_essential: bad argument");
    if (n < min_n || iters <= 0 || iters > (1 << 22) || n > (1 << 24))
        return vo_fail(ctx, VO_E_ARG, "vo_ransac_essential: need n >= %d and 0 < iters <= 4194304", min_n);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    EssWs w;
    int rc = ws_reserve(ctx, &ctx->mw->ransac_ws, &ctx->mw->ransac_ws_bytes, ess_ws_layout(nullptr, n, iters, &w));
    if (rc) return rc;
    ess_ws_layout(ctx->mw->ransac_ws, n, iters, &w);
    StageTimer t(ctx, VO_T_POSE);
    rc = xfer_h2d(ctx, w.p1, pts1, (size_t)n * 8);
    if (!rc) rc = xfer_h2d(ctx, w.p2, pts2, (size_t)n * 8);
    if (rc) return rc;
    const K4 K{ K4v[0], K4v[1], K4v[2], K4v[3] };
    const float thr2 = thr * thr;
    if (solver == 5) {
        if (int rc5 = hyp5_prepare(ctx)) return rc5;
        hipLaunchKernelGGL(k_ransac_hyp5, dim3(div_up(iters, 64)), dim3(64), FP_LDS_DOUBLES * sizeof(double), ctx->stream, w.p1, w.p2, n, K, iters, seed, w.rec, nullptr);
        hipLaunchKernelGGL(k_ransac_roots5, dim3(div_up(iters, 8)), dim3(256), 0, ctx->stream, w.rec, K, iters, w.E, w.F);
    }
    else
        hipLaunchKernelGGL(k_ransac_hyp, dim3(div_up(iters, 64)), dim3(64), 0, ctx->stream, w.p1, w.p2, n, K, iters, seed, w.E, w.F, nullptr);
    hipLaunchKernelGGL(k_ransac_score, dim3(div_up(iters, 4)), dim3(256), 0, ctx->stream, w.p1, w.p2, n, w.F, iters, thr2, w.counts, nullptr, min_n);
    hipLaunchKernelGGL(k_ransac_best, dim3(1), dim3(1024), 0, ctx->stream, w.counts, iters, w.best);
    hipLaunchKernelGGL(k_ransac_mask, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w.p1, w.p2, n, w.F, w.best, thr2, w.mask, nullptr, min_n);
    VO_CHECK_LAUNCH(ctx);
    VO_HIP(ctx, hipMemcpyAsync(ctx->pinned, w.best, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_out && (rc = xfer_d2h(ctx, mask_out, w.mask, (size_t)n))) return rc;
    if (counts_out && (rc = xfer_d2h(ctx, counts_out, w.counts, (size_t)iters * 4))) return rc;
    if ((rc = xfer_flush(ctx))) return rc;
    best2_out[0] = ((int32_t*)ctx->pinned)[0];
    best2_out[1] = ((int32_t*)ctx->pinned)[1];
    VO_HIP(ctx, hipMemcpy(E9_out, w.E + (size_t)best2_out[0] * 9, 72, hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_ransac_essential(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K4v, int iters, float thr,
                                   uint32_t seed, double* E9_out, uint8_t* mask_out, int32_t* counts_out, int32_t* best2_out)
{
    return ransac_essential(ctx, pts1, pts2, n, K4v, iters, thr, seed, E9_out, mask_out, counts_out, best2_out, 8);
}

extern "C" int vo_ransac_essential5(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K4v, int iters, float thr,
                                    uint32_t seed, double* E9_out, uint8_t* mask_out, int32_t* counts_out, int32_t* best2_out)
{
    return ransac_essential(ctx, pts1, pts2, n, K4v, iters, thr, seed, E9_out, mask_out, counts_out, best2_out, 5);
}

// winner's E (9 doubles) gathered on the device so that one flush brings everything home
__global__ void k_ransac_pick(const double* __restrict__ E_all, const int32_t* __restrict__ best, double* __restrict__ E9)
{
    if (threadIdx.x < 9) E9[threadIdx.x] = E_all[(size_t)best[0] * 9 + threadIdx.x];
}

// Monocular pair step (BASELINE config 5; no reference counterpart): the keypoints and descriptors two slots
// already hold -> brute-force Hamming kNN-2 -> ratio test + ordered compaction -> essential-matrix RANSAC on the
// surviving correspondences, every stage on the device.  mono_enqueue puts the whole chain on ctx->stream with the
// context's CURRENT match scratch (m_idx .. xy_b, m_count) and RANSAC workspace -- the main ones (vo_mono_pair: one
// host synchronisation at the end) or those of an asynchronous alternate (vo_mono_pair_begin / _end).
struct MonoStep { MonoWs w; float thr2; int min_n; };       // the step's workspace and what a tail kernel needs beside it

// The end of an asynchronous pair step as ONE launch (was three kernels and seven copy commands: at 8000 keypoints the
// monocular loop is bound by the host thread's queue entries): argmax of the hypotheses' inlier counts (most inliers, then the
// lowest index) -> the winner's E -> its inlier mask over the M correspondences -> the whole record -- M, winner, count, E,
// mask, the surviving index pairs and the second frame's keypoint positions -- written straight into the alternate's PINNED
// host record (one block: the record is 140 KB at 8000 keypoints).
__global__ void __launch_bounds__(1024) k_mono_finish(const int32_t* __restrict__ counts, int iters, const double* __restrict__ E_all,
                                                      const float* __restrict__ F_all, const float* __restrict__ p1, const float* __restrict__ p2,
                                                      int nq, const int* __restrict__ n_dev, int min_n, float thr2, const int32_t* __restrict__ mq,
                                                      const int32_t* __restrict__ mt, const float* __restrict__ xy_b, int nb, int want, size_t cap,
                                                      uint8_t* __restrict__ rec, size_t hdr)
{
    __shared__ long long s_key[16];
    int best, best_count;
    rs_block_argmax(counts, iters, s_key, best, best_count);
    const int m = *n_dev;
    int32_t* const h32 = (int32_t*)rec;
    if (threadIdx.x == 0) { h32[0] = m; h32[1] = best; h32[2] = best_count; }
    if (threadIdx.x < 9) ((double*)(rec + 64))[threadIdx.x] = E_all[(size_t)best * 9 + threadIdx.x];
    if (!want) return;
    uint8_t* const q = rec + hdr;
    const SampsonModel md{ p1, p2, min_n };
    float Fl[9];
    rs_winner_model<SampsonModel>(F_all, best, Fl);
    const int live = md.live(m);
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        q[i] = rs_inlier_of(md, Fl, i, live, thr2) ? 1 : 0;
        ((int32_t*)(q + cap))[i] = mq[i];
        ((int32_t*)(q + cap * 5))[i] = mt[i];
    }
    for (int i = threadIdx.x; i < nb; i += blockDim.x) ((float2*)(q + cap * 9))[i] = ((const float2*)xy_b)[i];
}

// fused_tail: the caller ends the chain with one kernel of its own (k_mono_finish, k_mono_pose_finish) that finds the winner;
// extra: bytes of scratch (o.w.scratch) that kernel needs
static int mono_enqueue(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, double ratio, int match_flags, const double* K4v, int iters, float thr, uint32_t seed,
                        int solver, MonoStep& o, bool fused_tail = false, size_t extra = 0)
{
    const int min_n = solver == 5 ? 6 : 8;
    const int nq = a.n_kp, cross = match_flags & VO_MATCH_CROSSCHECK;
    MonoWs& w = o.w;
    int rc = ws_reserve(ctx, &ctx->mw->ransac_ws, &ctx->mw->ransac_ws_bytes, mono_ws_layout(nullptr, nq, iters, extra, &w));
    if (rc) return rc;
    mono_ws_layout(ctx->mw->ransac_ws, nq, iters, extra, &w);
    {
        StageTimer t(ctx, VO_T_MATCH);
        if ((rc = match_knn2_slots(ctx, a, b, match_flags))) return rc;
        auto kern = cross ? k_ratio_compact<true> : k_ratio_compact<false>;
        hipLaunchKernelGGL(kern, dim3(1), dim3(nq > 512 ? 1024 : 256), 0, ctx->stream, ctx->mw->m_idx, ctx->mw->m_dist, nq, ratio, a.kp_xy, b.kp_xy,
                           ctx->mw->mq_idx, ctx->mw->mt_idx, ctx->mw->xy_a, ctx->mw->xy_b, ctx->mw->m_count,
                           cross ? (const uint32_t*)match_colmin(ctx->mw->m_dist, ctx->kp_cap) : nullptr, cross ? b.n_kp : 0,
                           (const uint8_t*)nullptr, (const uint8_t*)nullptr, 0);
    }
    {
        StageTimer t(ctx, VO_T_POSE);
        const K4 K{ K4v[0], K4v[1], K4v[2], K4v[3] };
        const float thr2 = o.thr2 = thr * thr;
        o.min_n = min_n;
        if (solver == 5) {
            if (int rc5 = hyp5_prepare(ctx)) return rc5;
            hipLaunchKernelGGL(k_ransac_hyp5, dim3(div_up(iters, 64)), dim3(64), FP_LDS_DOUBLES * sizeof(double), ctx->stream, ctx->mw->xy_a, ctx->mw->xy_b, nq, K, iters, seed, w.rec, ctx->mw->m_count);
            hipLaunchKernelGGL(k_ransac_roots5, dim3(div_up(iters, 8)), dim3(256), 0, ctx->stream, w.rec, K, iters, w.E, w.F);
        }
        else
            hipLaunchKernelGGL(k_ransac_hyp, dim3(div_up(iters, 64)), dim3(64), 0, ctx->stream, ctx->mw->xy_a, ctx->mw->xy_b, nq, K, iters, seed, w.E, w.F, ctx->mw->m_count);
        hipLaunchKernelGGL(k_ransac_score, dim3(div_up(iters, 4)), dim3(256), 0, ctx->stream, ctx->mw->xy_a, ctx->mw->xy_b, nq, w.F, iters, thr2, w.counts, ctx->mw->m_count, min_n);
        if (!fused_tail) {
            hipLaunchKernelGGL(k_ransac_best, dim3(1), dim3(1024), 0, ctx->stream, w.counts, iters, w.best);
            hipLaunchKernelGGL(k_ransac_mask, dim3(div_up(nq, 256)), dim3(256), 0, ctx->stream, ctx->mw->xy_a, ctx->mw->xy_b, nq, w.F, w.best, thr2, w.mask, ctx->mw->m_count, min_n);
            hipLaunchKernelGGL(k_ransac_pick, dim3(1), dim3(64), 0, ctx->stream, w.E, w.best, w.E9);
        }
        VO_CHECK_LAUNCH(ctx);
    }
    return VO_OK;
}

static int mono_check(vo_ctx* ctx, int slot_a, int slot_b, const double* K4v, int iters, int solver, const char* who)
{
    if (solver != 5 && solver != 8) return vo_fail(ctx, VO_E_ARG, "%s: solver is 5 (five-point) or 8 (eight-point)", who);
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !K4v)
        return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (iters <= 0 || iters > (1 << 22)) return vo_fail(ctx, VO_E_ARG, "%s: need 0 < iters <= 4194304", who);
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_kp || !b.has_kp) return vo_fail(ctx, VO_E_STATE, "%s: both slots need keypoints (vo_orb_detect_and_compute)", who);
    if (a.n_kp > 0 && b.n_kp < 2) return vo_fail(ctx, VO_E_ARG, "train set has fewer than 2 descriptors");
    return VO_OK;
}

extern "C" int vo_mono_pair_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                               uint32_t seed, int solver, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap)
{
    if (ctx && (!E9_out || !counts3)) return vo_fail(ctx, VO_E_ARG, "vo_mono_pair: bad argument");
    int rc = mono_check(ctx, slot_a, slot_b, K4v, iters, solver, "vo_mono_pair");
    if (!rc) rc = match_flags_check(ctx, match_flags, "vo_mono_pair");
    if (rc) return rc;
    const int min_n = solver == 5 ? 6 : 8;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    counts3[0] = counts3[1] = counts3[2] = 0;
    for (int k = 0; k < 9; k++) E9_out[k] = 0.0;
    if (a.n_kp == 0) return VO_OK;
    if ((mask_out || q_idx || t_idx) && cap < a.n_kp) return vo_fail(ctx, VO_E_CAP, "vo_mono_pair: outputs hold %d entries, %d keypoints", cap, a.n_kp);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    const int nq = a.n_kp;
    MonoStep o;
    if ((rc = mono_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, solver, o))) return rc;
    int32_t* h = (int32_t*)ctx->pinned;         // [0] M, [1..2] best, then E9 at byte 64
    VO_HIP(ctx, hipMemcpyAsync(h, ctx->mw->m_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(h + 1, o.w.best, 8, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync((uint8_t*)ctx->pinned + 64, o.w.E9, 72, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_out && (rc = xfer_d2h(ctx, mask_out, o.w.mask, (size_t)nq))) return rc;
    if (q_idx && (rc = xfer_d2h(ctx, q_idx, ctx->mw->mq_idx, (size_t)nq * 4))) return rc;
    if (t_idx && (rc = xfer_d2h(ctx, t_idx, ctx->mw->mt_idx, (size_t)nq * 4))) return rc;
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    counts3[0] = h[0]; counts3[1] = h[1]; counts3[2] = h[0] >= min_n ? h[2] : 0;
    memcpy(E9_out, (uint8_t*)ctx->pinned + 64, 72);
    return VO_OK;
}

extern "C" int vo_mono_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, const double* K4v, int iters, float thr, uint32_t seed,
                            int solver, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap)
{
    return vo_mono_pair_ex(ctx, slot_a, slot_b, ratio, 0, K4v, iters, thr, seed, solver, E9_out, counts3, mask_out, q_idx, t_idx, cap);
}

// ---- the same step, asynchronous: several pairs' chains in flight (each on an alternate's own stream and scratch) ----------
// A monocular stream is latency-bound when every pair is enqueued, waited for and only then followed by the next one (the
// five-point kernel alone runs 0.26 ms on 79 of the 1024 SIMDs).  Consecutive pairs do not depend on each other's result --
// only on the caller's decision which frame is the reference -- so a caller that knows the next frame may begin its pair
// before it collects this one's.  Results land in the alternate's pinned record; vo_mono_pair_end waits for its event only.
extern "C" int vo_mono_pair_begin_ex(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                                     uint32_t seed, int solver, int want_matches, int* ticket_out)
{
    if (ctx && !ticket_out) return vo_fail(ctx, VO_E_ARG, "vo_mono_pair_begin: bad argument");
    int rc = mono_check(ctx, slot_a, slot_b, K4v, iters, solver, "vo_mono_pair_begin");
    if (!rc) rc = match_flags_check(ctx, match_flags, "vo_mono_pair_begin");
    if (rc) return rc;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    int k;
    if ((rc = alt_open(ctx, vo_ctx::ALT_MONO, a, b, "vo_mono_pair_begin", &k))) return rc;
    vo_ctx::MonoAlt& p = ctx->mono_alt[k];
    memset(p.result, 0, MONO_HDR);
    p.nq = a.n_kp; p.nb = b.n_kp; p.min_n = solver == 5 ? 6 : 8; p.want = want_matches != 0; p.pose = false;
    if (a.n_kp > 0) {
        AltScope on_alt(ctx, p);
        MonoStep o;
        rc = mono_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, solver, o, true);
        if (!rc) {
            // (p.result is pinned host memory: the kernel writes the record across the link itself -- no copy command)
            hipLaunchKernelGGL(k_mono_finish, dim3(1), dim3(1024), 0, ctx->stream, o.w.counts, iters, o.w.E, o.w.F, ctx->mw->xy_a, ctx->mw->xy_b, a.n_kp,
                               ctx->mw->m_count, o.min_n, o.thr2, ctx->mw->mq_idx, ctx->mw->mt_idx, b.kp_xy, b.n_kp, p.want ? 1 : 0, (size_t)ctx->kp_cap,
                               p.result, MONO_HDR);
            if (hipGetLastError() != hipSuccess) rc = vo_fail(ctx, VO_E_HIP, "k_mono_finish: launch failed");
        }
    }
    if (rc) return rc;
    return alt_close(ctx, vo_ctx::ALT_MONO, k, a, b, ticket_out);
}

extern "C" int vo_mono_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, const double* K4v, int iters, float thr, uint32_t seed,
                                  int solver, int want_matches, int* ticket_out)
{
    return vo_mono_pair_begin_ex(ctx, slot_a, slot_b, ratio, 0, K4v, iters, thr, seed, solver, want_matches, ticket_out);
}

extern "C" int vo_mono_pair_end(vo_ctx* ctx, int ticket, double* E9_out, int32_t* counts3, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx,
                                float* xy_b_out, int cap)
{
    int rc = alt_ticket(ctx, vo_ctx::ALT_MONO, ticket, E9_out && counts3, "vo_mono_pair_end");
    if (rc) return rc;
    vo_ctx::MonoAlt& p = ctx->mono_alt[ticket];
    if (p.pose) return vo_fail(ctx, VO_E_STATE, "vo_mono_pair_end: ticket %d belongs to vo_mono_pose_pair_begin (end it with vo_mono_pose_pair_end)", ticket);
    if ((mask_out || q_idx || t_idx) && (!p.want || cap < p.nq)) return vo_fail(ctx, VO_E_CAP, "vo_mono_pair_end: outputs hold %d entries, %d keypoints (or the step was begun without want_matches)", cap, p.nq);
    if (xy_b_out && (!p.want || cap < p.nb)) return vo_fail(ctx, VO_E_CAP, "vo_mono_pair_end: xy_b_out holds %d entries, %d keypoints", cap, p.nb);
    if ((rc = alt_wait(ctx, p))) return rc;
    const int32_t* h = (const int32_t*)p.result;
    counts3[0] = h[0]; counts3[1] = h[1]; counts3[2] = h[0] >= p.min_n ? h[2] : 0;
    memcpy(E9_out, p.result + 64, 72);
    const uint8_t* q = p.result + MONO_HDR;
    const size_t kc = (size_t)ctx->kp_cap;
    if (mask_out) memcpy(mask_out, q, (size_t)p.nq);
    if (q_idx) memcpy(q_idx, q + kc, (size_t)p.nq * 4);
    if (t_idx) memcpy(t_idx, q + kc * 5, (size_t)p.nq * 4);
    if (xy_b_out) memcpy(xy_b_out, q + kc * 9, (size_t)p.nb * 8);
    return VO_OK;
}

// =========================================================================================
// Monocular pose recovery (vo_recover_pose, vo_mono_pose_pair / _begin / _end; no openVO counterpart): E -> (R, unit t) by the
// four-fold decomposition and a cheirality vote over EVERY inlier, the inliers' depths kept with the second frame's keypoints,
// and the ratio of this pair's baseline to the previous pair's from the keypoints the two pairs share.  One block (rp_tail)
// behind the winner's mask -- of the stand-alone entry (k_recover_pose) or of the fused pair step (k_mono_pose_finish):
//   pass 0   index check, inlier count (ballot + popcount), depth_b and the owner words cleared; one lane: 3x3 SVD, R1, R2, t
//   pass 1   the vote: both rotations with +t per inlier, four ballots per wave
//   pass 2   the winner's depths and parallax gate -> the valid set (ballot words in LDS), atomicMin of i on the owner word of
//            keypoint t_i (several correspondences may name one keypoint: the lowest i wins, whatever the thread timing)
//   pass 3   the owners write depth_b; depth_a[q_i] / z1_i of the shared keypoints as bit patterns
//   select   the lower median of those patterns exactly: eight 256-bin LDS histogram passes from the top byte down (positive
//            doubles order like their patterns)
// Float64, three-term sums left to right, no contraction: tests/mono_pose_ref.py restates it value for value.
// =========================================================================================
struct RpArgs : RpScratch {               // (the scratch z1, z2, ratio, owner: ransac_ws.h)
    const float *p1, *p2;                 // n x 2 pixels
    const int32_t *q, *t;                 // keypoint indices of the correspondences in frames a / b (both NULL: the identity)
    int na, nb;
    const double* depth_a;                // depths of frame a's keypoints in the previous pair's units (NULL: none)
    const uint32_t* serial_a;             // the serial word that goes with depth_a (NULL: not checked) ...
    uint32_t prev_serial;                 // ... and the serial it must hold
    double gate;                          // min_parallax_sin2
    K4 K;
    double* depth_b;                      // nb, written whole
    uint32_t* serial_b;                   // stamped with `serial` (NULL: no stamp)
    uint32_t serial;
    vo_mono_pose* rec;                    // pinned host memory
};

struct RpZ { double z1, z2, sin2; };
// depths along the two rays and the squared sine of the angle between them: z1 (R h1) + t = z2 h2
__device__ __forceinline__ RpZ rp_depths(const double* R, double t0, double t1, double t2, double x1, double y1, double hx, double hy)
{
    const double ax = (R[0] * x1 + R[1] * y1) + R[2], ay = (R[3] * x1 + R[4] * y1) + R[5], az = (R[6] * x1 + R[7] * y1) + R[8];
    const double nx = hy * t2 - t1, ny = t0 - hx * t2, nz = hx * t1 - hy * t0;          // h2 x t
    const double dx = ay - az * hy, dy = az * hx - ax, dz = ax * hy - ay * hx;          // (R h1) x h2
    const double dd = (dx * dx + dy * dy) + dz * dz;
    const double hh = (hx * hx + hy * hy) + 1.0;
    RpZ o;
    o.z1 = ((nx * dx + ny * dy) + nz * dz) / (dd > 1e-300 ? dd : 1e-300);
    o.z2 = (((o.z1 * ax + t0) * hx + (o.z1 * ay + t1) * hy) + (o.z1 * az + t2)) / hh;
    o.sin2 = dd / (((ax * ax + ay * ay) + az * az) * hh);
    return o;
}

__device__ __forceinline__ double rp_det3(const double* M)
{
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// s_mask: the inliers of the n correspondences as ballot words (written and synchronised by the caller); s_valid: as many words.
// M / best_iter go into the record as they come; best_count < 0: the number of inliers counted here.
__device__ void rp_tail(const RpArgs& A, int n, const double* E9, int M, int best_iter, int best_count, const unsigned long long* s_mask,
                        unsigned long long* s_valid)
{
    __shared__ double s_R[18], s_tw[3];
    __shared__ int s_cnt[16][4], s_votes[4], s_flags, s_winner, s_k;
    __shared__ unsigned int s_hist[256];
    __shared__ unsigned long long s_prefix;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const bool ident = A.q == nullptr;
    const double fx = A.K.fx, fy = A.K.fy, cx = A.K.cx, cy = A.K.cy;

    // ---- pass 0
    int bad = 0, cnt = 0;
    for (int i0 = wv * 64; i0 < n; i0 += blockDim.x) {
        const int i = i0 + lane;
        bool in = false;
        if (i < n) {
            in = (s_mask[i >> 6] >> (i & 63)) & 1ull;
            if (!ident) { const int qi = A.q[i], ti = A.t[i]; bad |= (qi < 0) | (qi >= A.na) | (ti < 0) | (ti >= A.nb); }
        }
        cnt += __popcll(__ballot(in));
    }
    for (int j = tid; j < A.nb; j += blockDim.x) { A.depth_b[j] = 0.0; A.owner[j] = 0x7fffffff; }
    if (lane == 0) s_cnt[wv][0] = cnt;
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        int n_inl = 0;
        for (int w = 0; w < nw; w++) n_inl += s_cnt[w][0];
        double E[9], U[9], sv[3], Vt[9];
        for (int k = 0; k < 9; k++) E[k] = E9[k];
        rs_svd3(E, U, sv, Vt);
        if (rp_det3(U) < 0.0) for (int k = 0; k < 9; k++) U[k] = -U[k];
        if (rp_det3(Vt) < 0.0) for (int k = 0; k < 9; k++) Vt[k] = -Vt[k];
        bool fin = true;
        for (int r = 0; r < 3; r++) {
            // U W = [u1, -u0, u2], U W^T = [-u1, u0, u2] (columns)
            const double w0 = U[r * 3 + 1], w1 = -U[r * 3], w2 = U[r * 3 + 2];
            for (int c = 0; c < 3; c++) {
                const double r1 = (w0 * Vt[c] + w1 * Vt[3 + c]) + w2 * Vt[6 + c];
                const double r2 = ((-w0) * Vt[c] + (-w1) * Vt[3 + c]) + w2 * Vt[6 + c];
                s_R[r * 3 + c] = r1; s_R[9 + r * 3 + c] = r2;
                fin = fin && isfinite(r1) && isfinite(r2);
            }
            fin = fin && isfinite(w2);
            s_tw[r] = w2;
        }
        int flags = bad ? 2 : 0;
        if (n_inl == 0 || !fin) flags |= 1;
        if (!(A.depth_a && (!A.serial_a || (A.prev_serial != 0 && *A.serial_a == A.prev_serial)))) flags |= 4;
        s_flags = flags;
        s_k = n_inl;
    }
    __syncthreads();
    const int flags = s_flags, n_inl = s_k;
    if (best_count < 0) best_count = n_inl;
    if (flags & 3) {                        // refused: nothing but zeros (depth_b is cleared already)
        for (int i = tid; i < n; i += blockDim.x) { A.z1[i] = 0.0; A.z2[i] = 0.0; }
        if (tid == 0) {
            vo_mono_pose* r = A.rec;
            r->M = M; r->best_iter = best_iter; r->best_count = best_count; r->winner = 0; r->n_depth = 0; r->n_shared = 0;
            r->flags = flags; r->serial = A.serial;
            for (int k = 0; k < 4; k++) r->votes4[k] = 0;
            for (int k = 0; k < 9; k++) { r->E[k] = E9[k]; r->R[k] = (k & 3) == 0 ? 1.0 : 0.0; }
            for (int k = 0; k < 3; k++) r->t[k] = 0.0;
            r->scale_rel = 0.0;
            if (A.serial_b) *A.serial_b = A.serial;
        }
        return;
    }

    // ---- pass 1: the vote
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i0 = wv * 64; i0 < n; i0 += blockDim.x) {
        const int i = i0 + lane;
        bool p1 = false, m1 = false, p2 = false, m2 = false;
        if (i < n && ((s_mask[i >> 6] >> (i & 63)) & 1ull)) {
            const float2 a = ((const float2*)A.p1)[i], b = ((const float2*)A.p2)[i];
            const double x1 = ((double)a.x - cx) / fx, y1 = ((double)a.y - cy) / fy, hx = ((double)b.x - cx) / fx, hy = ((double)b.y - cy) / fy;
            const RpZ u = rp_depths(s_R, s_tw[0], s_tw[1], s_tw[2], x1, y1, hx, hy);
            const RpZ v = rp_depths(s_R + 9, s_tw[0], s_tw[1], s_tw[2], x1, y1, hx, hy);
            p1 = u.z1 > 0.0 && u.z2 > 0.0; m1 = u.z1 < 0.0 && u.z2 < 0.0;
            p2 = v.z1 > 0.0 && v.z2 > 0.0; m2 = v.z1 < 0.0 && v.z2 < 0.0;
        }
        c0 += __popcll(__ballot(p1)); c1 += __popcll(__ballot(m1)); c2 += __popcll(__ballot(p2)); c3 += __popcll(__ballot(m2));
    }
    if (lane == 0) { s_cnt[wv][0] = c0; s_cnt[wv][1] = c1; s_cnt[wv][2] = c2; s_cnt[wv][3] = c3; }
    __syncthreads();
    if (tid == 0) {
        int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        for (int w = 0; w < nw; w++) { v0 += s_cnt[w][0]; v1 += s_cnt[w][1]; v2 += s_cnt[w][2]; v3 += s_cnt[w][3]; }
        s_votes[0] = v0; s_votes[1] = v1; s_votes[2] = v2; s_votes[3] = v3;
        const double tr1 = (s_R[0] + s_R[4]) + s_R[8], tr2 = (s_R[9] + s_R[13]) + s_R[17];
        // the largest vote; on a tie the rotation with the larger trace; then the lower index
        int best = 0, bv = v0;
        double bt = tr1;
        if (v1 > bv) { best = 1; bv = v1; }                                  // (same rotation as candidate 0: the trace cannot decide)
        if (v2 > bv || (v2 == bv && tr2 > bt)) { best = 2; bv = v2; bt = tr2; }
        if (v3 > bv || (v3 == bv && tr2 > bt)) { best = 3; bv = v3; bt = tr2; }
        s_winner = best;
        if (best & 1) for (int k = 0; k < 3; k++) s_tw[k] = -s_tw[k];
    }
    __syncthreads();
    const int winner = s_winner;
    const double* Rw = s_R + (winner >> 1) * 9;
    const double t0 = s_tw[0], t1 = s_tw[1], t2 = s_tw[2];

    // ---- pass 2: depths under the winner, the valid set, the owners
    int nd = 0;
    for (int i0 = wv * 64; i0 < n; i0 += blockDim.x) {
        const int i = i0 + lane;
        bool val = false;
        double z1 = 0.0, z2 = 0.0;
        if (i < n && ((s_mask[i >> 6] >> (i & 63)) & 1ull)) {
            const float2 a = ((const float2*)A.p1)[i], b = ((const float2*)A.p2)[i];
            const double x1 = ((double)a.x - cx) / fx, y1 = ((double)a.y - cy) / fy, hx = ((double)b.x - cx) / fx, hy = ((double)b.y - cy) / fy;
            const RpZ u = rp_depths(Rw, t0, t1, t2, x1, y1, hx, hy);
            z1 = u.z1; z2 = u.z2;
            val = z1 > 0.0 && z2 > 0.0 && u.sin2 >= A.gate;
            if (val) atomicMin(&A.owner[ident ? i : A.t[i]], i);
        }
        if (i < n) { A.z1[i] = z1; A.z2[i] = z2; }
        const unsigned long long bits = __ballot(val);
        if (lane == 0) s_valid[i0 >> 6] = bits;
        nd += __popcll(bits);
    }
    if (lane == 0) s_cnt[wv][0] = nd;
    __syncthreads();

    // ---- pass 3: the scatter, the ratios (thread tid has written z1 / z2 of the i it reads here)
    const bool use = !(flags & 4);
    int ns = 0;
    for (int i0 = wv * 64; i0 < n; i0 += blockDim.x) {
        const int i = i0 + lane;
        bool sh = false;
        unsigned long long pat = ~0ull;
        if (i < n && ((s_valid[i >> 6] >> (i & 63)) & 1ull)) {
            const int ti = ident ? i : A.t[i];
            if (__hip_atomic_load(&A.owner[ti], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i) A.depth_b[ti] = A.z2[i];
            if (use) {
                const double d = A.depth_a[ident ? i : A.q[i]];
                if (d > 0.0 && d <= 1.7976931348623157e308) { sh = true; pat = (unsigned long long)__double_as_longlong(d / A.z1[i]); }
            }
        }
        if (i < n) A.ratio[i] = pat;
        ns += __popcll(__ballot(sh));
    }
    if (lane == 0) s_cnt[wv][1] = ns;
    __syncthreads();
    int n_depth = 0, n_shared = 0;
    for (int w = 0; w < nw; w++) { n_depth += s_cnt[w][0]; n_shared += s_cnt[w][1]; }

    // ---- the lower median of the ratios: radix select on the 64-bit patterns
    if (tid == 0) { s_prefix = 0ull; s_k = (n_shared - 1) / 2; }
    if (n_shared > 0) {
        for (int pass = 0; pass < 8; pass++) {
            const int shift = 56 - 8 * pass;
            if (tid < 256) s_hist[tid] = 0u;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            for (int i = tid; i < n; i += blockDim.x) {
                const unsigned long long v = A.ratio[i];
                if (v != ~0ull && (pass == 0 || (v >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&s_hist[(unsigned)(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wv == 0) {                  // the bin that holds rank k: lane l owns bins 4l .. 4l + 3
                const unsigned h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
                const unsigned own = ((h0 + h1) + h2) + h3;
                unsigned incl = own;
                for (int o = 1; o < 64; o <<= 1) { const unsigned up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
                const unsigned excl = incl - own, k = (unsigned)s_k;
                if (k >= excl && k < incl) {
                    unsigned r = k - excl, bin = 4u * lane;
                    if (r >= h0) { r -= h0; bin++; if (r >= h1) { r -= h1; bin++; if (r >= h2) { r -= h2; bin++; } } }
                    s_prefix = prefix | ((unsigned long long)bin << shift);
                    s_k = (int)r;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) {
        vo_mono_pose* r = A.rec;
        r->M = M; r->best_iter = best_iter; r->best_count = best_count; r->winner = winner; r->n_depth = n_depth; r->n_shared = n_shared;
        r->flags = flags; r->serial = A.serial;
        for (int k = 0; k < 4; k++) r->votes4[k] = s_votes[k];
        for (int k = 0; k < 9; k++) { r->E[k] = E9[k]; r->R[k] = Rw[k]; }
        r->t[0] = t0; r->t[1] = t1; r->t[2] = t2;
        r->scale_rel = n_shared > 0 ? __longlong_as_double((long long)s_prefix) : 0.0;
        if (A.serial_b) *A.serial_b = A.serial;
    }
}

static inline size_t rp_lds_bytes(int n) { return (size_t)((n + 63) >> 6) * 16; }

__global__ void __launch_bounds__(1024) k_recover_pose(RpArgs A, int n, const double* __restrict__ E9, const uint8_t* __restrict__ mask)
{
    extern __shared__ unsigned long long s_bits[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwords = (n + 63) >> 6;
    for (int i0 = wv * 64; i0 < n; i0 += blockDim.x) {
        const int i = i0 + lane;
        const unsigned long long bits = __ballot(i < n && (!mask || mask[i] != 0));
        if (lane == 0) s_bits[i0 >> 6] = bits;
    }
    __syncthreads();
    rp_tail(A, n, E9, n, -1, -1, s_bits, s_bits + nwords);
}

// The end of a monocular pose step as ONE launch: argmax of the hypotheses' inlier counts, the winner's E and its inlier mask
// (the mask as ballot words in LDS instead of bytes in a record), then rp_tail on the M surviving correspondences.  Nothing per
// match crosses the link: the record is a vo_mono_pose.
__global__ void __launch_bounds__(1024) k_mono_pose_finish(const int32_t* __restrict__ counts, int iters, const double* __restrict__ E_all,
                                                           const float* __restrict__ F_all, int nq, const int* __restrict__ n_dev, int min_n,
                                                           float thr2, RpArgs A)
{
    extern __shared__ unsigned long long s_bits[];
    __shared__ long long s_key[16];
    __shared__ double s_E[9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int best, best_count;
    rs_block_argmax(counts, iters, s_key, best, best_count);
    int m = *n_dev;
    m = m < 0 ? 0 : (m > nq ? nq : m);      // (the LDS words and the scratch are sized for nq)
    if (threadIdx.x < 9) s_E[threadIdx.x] = E_all[(size_t)best * 9 + threadIdx.x];
    const SampsonModel md{ A.p1, A.p2, min_n };
    float Fl[9];
    rs_winner_model<SampsonModel>(F_all, best, Fl);
    const int live = md.live(m);
    for (int i0 = wv * 64; i0 < m; i0 += blockDim.x) {
        const unsigned long long bits = __ballot(rs_inlier_of(md, Fl, i0 + lane, live, thr2));
        if (lane == 0) s_bits[i0 >> 6] = bits;
    }
    __syncthreads();
    rp_tail(A, m, s_E, m, best, live ? best_count : 0, s_bits, s_bits + ((nq + 63) >> 6));
}

static int rp_check_out(vo_ctx* ctx, const vo_mono_pose* r, const char* who)
{
    if (r->flags & 2) return vo_fail(ctx, VO_E_STATE, "%s: a keypoint index lies outside its frame: the step is refused", who);
    return VO_OK;
}

static void rp_rec_clear(vo_mono_pose* r)
{
    memset(r, 0, sizeof(vo_mono_pose));
    r->R[0] = r->R[4] = r->R[8] = 1.0;
    r->flags = 1 | 4;
}

extern "C" int vo_recover_pose(vo_ctx* ctx, const double* E9, const float* pts1, const float* pts2, const uint8_t* mask, int n, const double* K4v,
                               const int32_t* q_idx, const int32_t* t_idx, int na, int nb, const double* depth_a, double min_parallax_sin2,
                               vo_mono_pose* out, double* depth_b, double* z1_out, double* z2_out)
{
    if (!ctx || !E9 || !pts1 || !pts2 || !K4v || !out || (q_idx == nullptr) != (t_idx == nullptr) || !(min_parallax_sin2 >= 0.0) ||
        !(K4v[0] > 0.0) || !(K4v[1] > 0.0))
        return vo_fail(ctx, VO_E_ARG, "vo_recover_pose: bad argument");
    if (n < 1 || n > 65536) return vo_fail(ctx, VO_E_CAP, "vo_recover_pose: need 1 <= n <= 65536");
    if (!q_idx) na = nb = n;
    if (na < 1 || nb < 1 || na > (1 << 24) || nb > (1 << 24)) return vo_fail(ctx, VO_E_ARG, "vo_recover_pose: need 1 <= na, nb <= 16777216");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    RecoverWs w;
    int rc = ws_reserve(ctx, &ctx->mw->ransac_ws, &ctx->mw->ransac_ws_bytes, recover_ws_layout(nullptr, n, na, nb, &w));
    if (rc) return rc;
    recover_ws_layout(ctx->mw->ransac_ws, n, na, nb, &w);
    StageTimer t(ctx, VO_T_POSE);
    rc = xfer_h2d(ctx, w.E, E9, 72);
    if (!rc) rc = xfer_h2d(ctx, w.p1, pts1, (size_t)n * 8);
    if (!rc) rc = xfer_h2d(ctx, w.p2, pts2, (size_t)n * 8);
    if (!rc && mask) rc = xfer_h2d(ctx, w.mask, mask, (size_t)n);
    if (!rc && q_idx) rc = xfer_h2d(ctx, w.q, q_idx, (size_t)n * 4);
    if (!rc && t_idx) rc = xfer_h2d(ctx, w.t, t_idx, (size_t)n * 4);
    if (!rc && depth_a) rc = xfer_h2d(ctx, w.da, depth_a, (size_t)na * 8);
    if (rc) return rc;
    vo_mono_pose* rec = (vo_mono_pose*)ctx->pinned;
    rp_rec_clear(rec);
    RpArgs A{};
    A.p1 = w.p1; A.p2 = w.p2; A.q = q_idx ? w.q : nullptr; A.t = t_idx ? w.t : nullptr; A.na = na; A.nb = nb;
    A.depth_a = depth_a ? w.da : nullptr; A.serial_a = nullptr; A.prev_serial = 0; A.gate = min_parallax_sin2;
    A.K = K4{ K4v[0], K4v[1], K4v[2], K4v[3] };
    A.depth_b = w.db; A.serial_b = nullptr; A.serial = 0; A.rec = rec;
    rp_scratch_layout(w.scratch, n, nb, &A);
    hipLaunchKernelGGL(k_recover_pose, dim3(1), dim3(1024), rp_lds_bytes(n), ctx->stream, A, n, w.E, mask ? w.mask : nullptr);
    VO_CHECK_LAUNCH(ctx);
    if (depth_b && (rc = xfer_d2h(ctx, depth_b, w.db, (size_t)nb * 8))) return rc;
    if (z1_out && (rc = xfer_d2h(ctx, z1_out, A.z1, (size_t)n * 8))) return rc;
    if (z2_out && (rc = xfer_d2h(ctx, z2_out, A.z2, (size_t)n * 8))) return rc;
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    *out = *rec;
    return rp_check_out(ctx, out, "vo_recover_pose");
}

// ---- the fused step --------------------------------------------------------------------------------------------------------
static int mono_pose_check(vo_ctx* ctx, int slot_a, int slot_b, int match_flags, const double* K4v, int iters, int solver, double gate,
                           const void* out, const char* who)
{
    if (ctx && (!out || !(gate >= 0.0) || slot_a == slot_b))
        return vo_fail(ctx, VO_E_ARG, "%s: bad argument (two different slots, min_parallax_sin2 >= 0)", who);
    int rc = mono_check(ctx, slot_a, slot_b, K4v, iters, solver, who);
    if (!rc) rc = match_flags_check(ctx, match_flags, who);
    if (rc) return rc;
    if (!(K4v[0] > 0.0) || !(K4v[1] > 0.0)) return vo_fail(ctx, VO_E_ARG, "%s: need positive focal lengths", who);
    if (rp_lds_bytes(ctx->slots[slot_a].n_kp) > 48 * 1024) return vo_fail(ctx, VO_E_CAP, "%s: %d keypoints exceed the step's LDS", who, ctx->slots[slot_a].n_kp);
    return VO_OK;
}

static uint32_t mono_next_serial(vo_ctx* ctx)
{
    if (++ctx->mono_serial_next == 0) ctx->mono_serial_next = 1;
    return ctx->mono_serial_next;
}

// The chain of mono_enqueue on ctx->stream (the main one or an alternate's) with k_mono_pose_finish as its tail.  The tail alone
// is ordered behind the step that writes slot a's depths, behind an earlier writer of slot b's and behind the steps still
// reading slot b: the kNN and the RANSAC in front of it overlap them.  `rec`: pinned host memory.
static int mono_pose_enqueue(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, double ratio, int match_flags, const double* K4v, int iters, float thr, uint32_t seed,
                             int solver, uint32_t prev_serial, double gate, uint32_t serial, vo_mono_pose* rec)
{
    MonoStep o;
    RpArgs A{};
    int rc = mono_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, solver, o, true, rp_scratch_layout(nullptr, a.n_kp, b.n_kp, &A));
    if (rc) return rc;
    if (a.depth_writer) VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, a.depth_writer, 0));
    if (b.depth_writer) VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, b.depth_writer, 0));
    for (hipEvent_t r : b.readers) if (r) VO_HIP(ctx, hipStreamWaitEvent(ctx->stream, r, 0));
    A.p1 = ctx->mw->xy_a; A.p2 = ctx->mw->xy_b; A.q = ctx->mw->mq_idx; A.t = ctx->mw->mt_idx; A.na = a.n_kp; A.nb = b.n_kp;
    // depths of slot a are offered only under the serial the HOST still holds for them (a refill clears it at once)
    const bool offer = prev_serial != 0 && a.mono_serial == prev_serial;
    A.depth_a = offer ? a.mono_depth : nullptr; A.serial_a = a.mono_serial_dev; A.prev_serial = prev_serial; A.gate = gate;
    A.K = K4{ K4v[0], K4v[1], K4v[2], K4v[3] };
    A.depth_b = b.mono_depth; A.serial_b = b.mono_serial_dev; A.serial = serial; A.rec = rec;
    rp_scratch_layout(o.w.scratch, a.n_kp, b.n_kp, &A);
    StageTimer t(ctx, VO_T_POSE);
    hipLaunchKernelGGL(k_mono_pose_finish, dim3(1), dim3(1024), rp_lds_bytes(a.n_kp), ctx->stream, o.w.counts, iters, o.w.E, o.w.F, a.n_kp,
                       ctx->mw->m_count, o.min_n, o.thr2, A);
    VO_CHECK_LAUNCH(ctx);
    b.mono_serial = serial;
    return VO_OK;
}

extern "C" int vo_mono_pose_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                                 uint32_t seed, int solver, uint32_t prev_serial, double min_parallax_sin2, vo_mono_pose* out)
{
    int rc = mono_pose_check(ctx, slot_a, slot_b, match_flags, K4v, iters, solver, min_parallax_sin2, out, "vo_mono_pose_pair");
    if (rc) return rc;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    rp_rec_clear(out);
    if (a.n_kp == 0) { b.mono_serial = 0; return VO_OK; }      // nothing to match: no step, no depths
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    vo_mono_pose* rec = (vo_mono_pose*)ctx->pinned;
    rp_rec_clear(rec);
    if ((rc = mono_pose_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, solver, prev_serial, min_parallax_sin2,
                                mono_next_serial(ctx), rec)))
        return rc;
    if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
    b.depth_writer = nullptr;
    *out = *rec;
    return rp_check_out(ctx, out, "vo_mono_pose_pair");
}

extern "C" int vo_mono_pose_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                                       uint32_t seed, int solver, uint32_t prev_serial, double min_parallax_sin2, int* ticket_out,
                                       uint32_t* serial_out)
{
    int rc = mono_pose_check(ctx, slot_a, slot_b, match_flags, K4v, iters, solver, min_parallax_sin2, ticket_out, "vo_mono_pose_pair_begin");
    if (rc) return rc;
    if (!serial_out) return vo_fail(ctx, VO_E_ARG, "vo_mono_pose_pair_begin: bad argument");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    int k;
    if ((rc = alt_open(ctx, vo_ctx::ALT_MONO, a, b, "vo_mono_pose_pair_begin", &k))) return rc;
    vo_ctx::MonoAlt& p = ctx->mono_alt[k];
    rp_rec_clear((vo_mono_pose*)p.result);
    p.nq = a.n_kp; p.nb = b.n_kp; p.min_n = solver == 5 ? 6 : 8; p.want = false; p.pose = true;
    *serial_out = 0;
    if (a.n_kp > 0) {
        const uint32_t serial = mono_next_serial(ctx);
        AltScope on_alt(ctx, p);
        rc = mono_pose_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, solver, prev_serial, min_parallax_sin2,
                               serial, (vo_mono_pose*)p.result);
        if (!rc) *serial_out = serial;
    } else
        b.mono_serial = 0;
    if (rc) return rc;
    if ((rc = alt_close(ctx, vo_ctx::ALT_MONO, k, a, b, ticket_out))) return rc;
    if (a.n_kp > 0) b.depth_writer = p.done;
    return VO_OK;
}

extern "C" int vo_mono_pose_pair_end(vo_ctx* ctx, int ticket, vo_mono_pose* out)
{
    int rc = alt_ticket(ctx, vo_ctx::ALT_MONO, ticket, out != nullptr, "vo_mono_pose_pair_end");
    if (rc) return rc;
    vo_ctx::MonoAlt& p = ctx->mono_alt[ticket];
    if (!p.pose) return vo_fail(ctx, VO_E_STATE, "vo_mono_pose_pair_end: ticket %d belongs to vo_mono_pair_begin (end it with vo_mono_pair_end)", ticket);
    if ((rc = alt_wait(ctx, p))) return rc;
    *out = *(const vo_mono_pose*)p.result;
    return rp_check_out(ctx, out, "vo_mono_pose_pair_end");
}

extern "C" int vo_download_mono_depth(vo_ctx* ctx, int slot, double* out, uint32_t* serial_out)
{
    if (!ctx || slot < 0 || slot >= VO_NUM_SLOTS || !serial_out) return vo_fail(ctx, VO_E_ARG, "vo_download_mono_depth: bad argument");
    FrameSlot& f = ctx->slots[slot];
    if (!f.has_kp) return vo_fail(ctx, VO_E_STATE, "vo_download_mono_depth: the slot has no keypoints");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    *serial_out = 0;
    if (f.mono_serial == 0) {
        if (out) memset(out, 0, (size_t)f.n_kp * 8);
        return VO_OK;
    }
    if (f.depth_writer) { VO_HIP(ctx, hipEventSynchronize(f.depth_writer)); f.depth_writer = nullptr; }
    int rc = xfer_d2h(ctx, serial_out, f.mono_serial_dev, 4);
    if (!rc && out) rc = xfer_d2h(ctx, out, f.mono_depth, (size_t)f.n_kp * 8);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// =========================================================================================
// RANSAC solvePnP hypothesis generation + reprojection scoring (the north star's "solvePnP
// hypothesis-scoring loop").  No openVO counterpart either; same structure as above:
//   k_pnp_hyp     one lane per hypothesis: 4 hash-sampled correspondences, P3P on three of them in
//                 float64 (depths along the bearings; singular member of the two-conic pencil by a
//                 bisected cubic root -- only + - * / sqrt; <= 4 poses, Gauss-Newton polish), the fourth
//                 picks the pose; P = K [R|t] rounded to float32
//   k_pnp_score   one wave per hypothesis; division-free reprojection test in float32
//                 ((xc - u zc)^2 + (yc - v zc)^2 < thr^2 zc^2, zc > 0), ballot + popcount
//   k_pnp_finish  (vo_pnp_pair) one block: winner, its mask, Gauss-Newton refinement on the mask, the record into pinned memory
// =========================================================================================
__device__ __forceinline__ double pn_det3(const double m[3][3])
{
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

__device__ double pn_det3_col(const double A[3][3], const double B[3][3], int c)
{
    double m[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m[i][j] = j == c ? B[i][j] : A[i][j];
    return pn_det3(m);
}

__device__ __forceinline__ double pn_cubic(const double* c, double g) { return ((c[3] * g + c[2]) * g + c[1]) * g + c[0]; }

__device__ double pn_cubic_root(const double* c)
{
    double m = fabs(c[2]);
    if (fabs(c[1]) > m) m = fabs(c[1]);
    if (fabs(c[0]) > m) m = fabs(c[0]);
    double hi = 1.0 + m / fabs(c[3]), lo = -hi;
    double flo = pn_cubic(c, lo);
    for (int it = 0; it < 80; it++) {
        const double mid = 0.5 * (lo + hi), fm = pn_cubic(c, mid);
        if ((fm < 0.0) == (flo < 0.0)) { lo = mid; flo = fm; } else hi = mid;
    }
    double g = 0.5 * (lo + hi);
    for (int it = 0; it < 2; it++) {
        const double d = (3.0 * c[3] * g + 2.0 * c[2]) * g + c[1];
        if (d != 0.0) g -= pn_cubic(c, g) / d;
    }
    return g;
}

__device__ bool pn_null_vec(const double M[3][3], double s, double* e)
{
    double r[3][3], c[3][3], best = -1.0;
    int bi = 0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r[i][j] = M[i][j] - (i == j ? s : 0.0);
    rs_cross3(r[0], r[1], c[0]);
    rs_cross3(r[0], r[2], c[1]);
    rs_cross3(r[1], r[2], c[2]);
    for (int k = 0; k < 3; k++) {
        const double n2 = c[k][0] * c[k][0] + c[k][1] * c[k][1] + c[k][2] * c[k][2];
        if (n2 > best) { best = n2; bi = k; }
    }
    if (!(best > 0.0)) return false;
    const double inv = 1.0 / sqrt(best);
    for (int k = 0; k < 3; k++) e[k] = c[bi][k] * inv;
    return true;
}

// y: 3 unit bearings, x: 3 points (rows); Rs/ts receive up to 4 poses
__device__ int pn_p3p(const double* y, const double* x, double* Rs, double* ts)
{
    const double *y1 = y, *y2 = y + 3, *y3 = y + 6, *x1 = x, *x2 = x + 3, *x3 = x + 6;
    const double b12 = y1[0] * y2[0] + y1[1] * y2[1] + y1[2] * y2[2];
    const double b13 = y1[0] * y3[0] + y1[1] * y3[1] + y1[2] * y3[2];
    const double b23 = y2[0] * y3[0] + y2[1] * y3[1] + y2[2] * y3[2];
    double d12[3], d13[3], d23[3], dx[3];
    for (int k = 0; k < 3; k++) { d12[k] = x1[k] - x2[k]; d13[k] = x1[k] - x3[k]; d23[k] = x2[k] - x3[k]; }
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    rs_cross3(d12, d13, dx);
    const double area2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2];
    if (!(a12 > 0.0) || !(a13 > 0.0) || !(a23 > 0.0) || !(area2 > 1e-24 * a12 * a13)) return 0;

    const double D1[3][3] = { { a23, -a23 * b12, 0.0 }, { -a23 * b12, a23 - a12, a12 * b23 }, { 0.0, a12 * b23, -a12 } };
    const double D2[3][3] = { { a23, 0.0, -a23 * b13 }, { 0.0, -a13, a13 * b23 }, { -a23 * b13, a13 * b23, a23 - a13 } };
    double c[4];
    c[0] = pn_det3(D1);
    c[3] = pn_det3(D2);
    c[1] = (pn_det3_col(D1, D2, 0) + pn_det3_col(D1, D2, 1)) + pn_det3_col(D1, D2, 2);
    c[2] = (pn_det3_col(D2, D1, 0) + pn_det3_col(D2, D1, 1)) + pn_det3_col(D2, D1, 2);
    double D0[3][3];
    if (fabs(c[3]) >= fabs(c[0])) {
        if (c[3] == 0.0) return 0;
        const double g = pn_cubic_root(c);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) D0[i][j] = D1[i][j] + g * D2[i][j];
    } else {
        const double cr[4] = { c[3], c[2], c[1], c[0] };
        const double g = pn_cubic_root(cr);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) D0[i][j] = g * D1[i][j] + D2[i][j];
    }
    const double tr = (D0[0][0] + D0[1][1]) + D0[2][2];
    const double m2 = ((D0[0][0] * D0[1][1] - D0[0][1] * D0[0][1]) + (D0[0][0] * D0[2][2] - D0[0][2] * D0[0][2])) +
                      (D0[1][1] * D0[2][2] - D0[1][2] * D0[1][2]);
    if (!(m2 < 0.0)) return 0;
    const double disc = tr * tr - 4.0 * m2;
    const double s1 = 0.5 * (tr + (tr >= 0.0 ? 1.0 : -1.0) * sqrt(disc));
    const double s2 = m2 / s1;
    double e1[3], e2[3];
    if (!pn_null_vec(D0, s1, e1) || !pn_null_vec(D0, s2, e2)) return 0;
    const double s = sqrt(-s2 / s1);

    int ns = 0;
    for (int sg = 0; sg < 2; sg++) {
        double p[3];
        for (int k = 0; k < 3; k++) p[k] = e1[k] + (sg ? -s : s) * e2[k];
        if (!(fabs(p[0]) > 1e-12)) continue;
        const double w0 = -p[1] / p[0], w1 = -p[2] / p[0];
        const double A = a23 * w1 * w1 - a12;
        const double B = (2.0 * a23 * w0 * w1 - 2.0 * a23 * b12 * w1) + 2.0 * a12 * b23;
        const double C = ((a23 * w0 * w0 - 2.0 * a23 * b12 * w0) + a23) - a12;
        double tau[2];
        int nt = 0;
        if (fabs(A) > 1e-14 * (fabs(B) + fabs(C))) {
            const double dq = B * B - 4.0 * A * C;
            if (dq >= 0.0) {
                const double sq = sqrt(dq);
                tau[0] = (-B + sq) / (2.0 * A);
                tau[1] = (-B - sq) / (2.0 * A);
                nt = 2;
            }
        } else if (B != 0.0) {
            tau[0] = -C / B;
            nt = 1;
        }
        for (int q = 0; q < nt; q++) {
            const double t = tau[q];
            if (!(t > 0.0)) continue;
            const double den = (1.0 + t * t) - 2.0 * b23 * t;
            if (!(den > 0.0)) continue;
            double l2 = sqrt(a23 / den), l3 = t * l2, l1 = (w0 + w1 * t) * l2;
            if (!(l1 > 0.0)) continue;
            for (int it = 0; it < 3; it++) {
                const double r0 = ((l1 * l1 + l2 * l2) - 2.0 * b12 * l1 * l2) - a12;
                const double r1 = ((l1 * l1 + l3 * l3) - 2.0 * b13 * l1 * l3) - a13;
                const double r2 = ((l2 * l2 + l3 * l3) - 2.0 * b23 * l2 * l3) - a23;
                const double J[3][3] = { { 2.0 * l1 - 2.0 * b12 * l2, 2.0 * l2 - 2.0 * b12 * l1, 0.0 },
                                         { 2.0 * l1 - 2.0 * b13 * l3, 0.0, 2.0 * l3 - 2.0 * b13 * l1 },
                                         { 0.0, 2.0 * l2 - 2.0 * b23 * l3, 2.0 * l3 - 2.0 * b23 * l2 } };
                const double dj = pn_det3(J);
                if (dj == 0.0) break;
                const double rr[3][3] = { { r0, r0, r0 }, { r1, r1, r1 }, { r2, r2, r2 } };
                const double n0 = pn_det3_col(J, rr, 0), n1 = pn_det3_col(J, rr, 1), n2 = pn_det3_col(J, rr, 2);
                l1 -= n0 / dj; l2 -= n1 / dj; l3 -= n2 / dj;
            }
            if (!(l1 > 0.0) || !(l2 > 0.0) || !(l3 > 0.0)) continue;
            double ya[3], yb[3], yc[3];
            for (int k = 0; k < 3; k++) { ya[k] = l1 * y1[k] - l2 * y2[k]; yb[k] = l1 * y1[k] - l3 * y3[k]; }
            rs_cross3(ya, yb, yc);
            const double X[3][3] = { { d12[0], d13[0], dx[0] }, { d12[1], d13[1], dx[1] }, { d12[2], d13[2], dx[2] } };
            const double dX = pn_det3(X);
            if (dX == 0.0) continue;
            double Xi[3][3];
            Xi[0][0] = (X[1][1] * X[2][2] - X[1][2] * X[2][1]) / dX;
            Xi[0][1] = (X[0][2] * X[2][1] - X[0][1] * X[2][2]) / dX;
            Xi[0][2] = (X[0][1] * X[1][2] - X[0][2] * X[1][1]) / dX;
            Xi[1][0] = (X[1][2] * X[2][0] - X[1][0] * X[2][2]) / dX;
            Xi[1][1] = (X[0][0] * X[2][2] - X[0][2] * X[2][0]) / dX;
            Xi[1][2] = (X[0][2] * X[1][0] - X[0][0] * X[1][2]) / dX;
            Xi[2][0] = (X[1][0] * X[2][1] - X[1][1] * X[2][0]) / dX;
            Xi[2][1] = (X[0][1] * X[2][0] - X[0][0] * X[2][1]) / dX;
            Xi[2][2] = (X[0][0] * X[1][1] - X[0][1] * X[1][0]) / dX;
            double* R = Rs + 9 * ns;
            double* tt = ts + 3 * ns;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[i * 3 + j] = (ya[i] * Xi[0][j] + yb[i] * Xi[1][j]) + yc[i] * Xi[2][j];
            for (int i = 0; i < 3; i++) tt[i] = l1 * y1[i] - ((R[i * 3] * x1[0] + R[i * 3 + 1] * x1[1]) + R[i * 3 + 2] * x1[2]);
            ns++;
        }
    }
    return ns;
}

// column c of P = K [R | t], rounded to float32 (Rt, P: 3 x 4, row-major)
__device__ __forceinline__ void pnp_project_col(const K4& K, const double* Rt, int c, float* P)
{
    P[c] = (float)(K.fx * Rt[c] + K.cx * Rt[8 + c]);
    P[4 + c] = (float)(K.fy * Rt[4 + c] + K.cy * Rt[8 + c]);
    P[8 + c] = (float)Rt[8 + c];
}

__device__ __forceinline__ void pnp_project(const K4& K, const double* Rt, float* P)
{
    for (int c = 0; c < 4; c++) pnp_project_col(K, Rt, c, P);
}

__global__ void __launch_bounds__(64) k_pnp_hyp(const float* __restrict__ X, const float* __restrict__ uv, int n, K4 K, int iters,
                                                uint32_t seed, double* __restrict__ Rt_out, float* __restrict__ P_out,
                                                const int* __restrict__ n_dev)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= iters) return;
    // n_dev (may be NULL): the number of correspondences when only the device knows it (vo_pnp_pair: what k_pnp_prep kept);
    // fewer than 4 give no pose: an all-zero hypothesis that scores no inlier
    if (n_dev) {
        n = *n_dev;
        if (n < 4) {
            for (int k = 0; k < 12; k++) { Rt_out[(size_t)h * 12 + k] = 0.0; P_out[(size_t)h * 12 + k] = 0.0f; }
            return;
        }
    }
    int idx[4];
    rs_sample_distinct<4>(seed, h, n, idx);
    double y[9], x[9], Rs[36], ts[12];
    for (int s = 0; s < 3; s++) {
        const int i = idx[s];
        const double a = ((double)uv[2 * i] - K.cx) / K.fx, b = ((double)uv[2 * i + 1] - K.cy) / K.fy;
        const double inv = 1.0 / sqrt((a * a + b * b) + 1.0);
        y[3 * s] = a * inv; y[3 * s + 1] = b * inv; y[3 * s + 2] = inv;
        for (int k = 0; k < 3; k++) x[3 * s + k] = (double)X[3 * i + k];
    }
    const int ns = pn_p3p(y, x, Rs, ts);
    const int i4 = idx[3];
    const double u4 = ((double)uv[2 * i4] - K.cx) / K.fx, v4 = ((double)uv[2 * i4 + 1] - K.cy) / K.fy;
    const double x4[3] = { (double)X[3 * i4], (double)X[3 * i4 + 1], (double)X[3 * i4 + 2] };
    int best = -1;
    double beste = 0.0;
    for (int s = 0; s < ns; s++) {
        const double* R = Rs + 9 * s;
        const double* t = ts + 3 * s;
        const double xc = ((R[0] * x4[0] + R[1] * x4[1]) + R[2] * x4[2]) + t[0];
        const double yc = ((R[3] * x4[0] + R[4] * x4[1]) + R[5] * x4[2]) + t[1];
        const double zc = ((R[6] * x4[0] + R[7] * x4[1]) + R[8] * x4[2]) + t[2];
        if (!(zc > 0.0)) continue;
        const double du = xc / zc - u4, dv = yc / zc - v4, e = du * du + dv * dv;
        if (best < 0 || e < beste) { best = s; beste = e; }
    }
    double Rt[12];
    float P[12];
    if (best < 0) {
        for (int k = 0; k < 12; k++) { Rt[k] = 0.0; P[k] = 0.0f; }
    } else {
        const double* R = Rs + 9 * best;
        const double* t = ts + 3 * best;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Rt[r * 4 + c] = R[r * 3 + c]; Rt[r * 4 + 3] = t[r]; }
        pnp_project(K, Rt, P);
    }
    for (int k = 0; k < 12; k++) { Rt_out[(size_t)h * 12 + k] = Rt[k]; P_out[(size_t)h * 12 + k] = P[k]; }
}

__device__ __forceinline__ bool reproj_inlier(const float* P, float X, float Y, float Z, float u, float v, float thr2)
{
    const float xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const float yc = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const float zc = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    const float du = xc - u * zc, dv = yc - v * zc;
    const float e = du * du + dv * dv;
    const float lim = thr2 * (zc * zc);
    return zc > 0.0f && e < lim;
}

struct ReprojModel {                        // P (12 floats) on 3-D points and their pixels
    static constexpr int W = 12;
    const float *X, *uv;
    __device__ __forceinline__ int live(int n) const { return n < 4 ? 0 : n; }
    __device__ __forceinline__ bool inlier(const float* P, int i, float thr2) const
    {
        const float2 b = ((const float2*)uv)[i];
        return reproj_inlier(P, X[3 * i], X[3 * i + 1], X[3 * i + 2], b.x, b.y, thr2);
    }
};

__global__ void __launch_bounds__(256) k_pnp_score(const float* __restrict__ X, const float* __restrict__ uv, int n,
                                                  const float* __restrict__ P_all, int iters, float thr2, int32_t* __restrict__ counts,
                                                  const int* __restrict__ n_dev)
{
    rs_score_wave(ReprojModel{ X, uv }, n, P_all, iters, thr2, counts, n_dev);
}

__global__ void k_pnp_mask(const float* __restrict__ X, const float* __restrict__ uv, int n, const float* __restrict__ P_all,
                           const int32_t* __restrict__ best, float thr2, uint8_t* __restrict__ mask)
{
    rs_mask_point(ReprojModel{ X, uv }, n, P_all, best, thr2, mask, nullptr);
}

extern "C" int vo_ransac_pnp(vo_ctx* ctx, const float* pts3d, const float* pts2d, int n, const double* K4v, int iters, float thr,
                             uint32_t seed, double* Rt12_out, uint8_t* mask_out, int32_t* counts_out, int32_t* best2_out)
{
    if (!ctx || !pts3d || !pts2d || !K4v || !Rt12_out || !best2_out) return vo_fail(ctx, VO_E_ARG, "vo_ransac_pnp: bad argument");
    if (n < 4 || iters <= 0 || iters > (1 << 22) || n > (1 << 24)) return vo_fail(ctx, VO_E_ARG, "vo_ransac_pnp: need n >= 4 and 0 < iters <= 4194304");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    PnpHostWs w;
    int rc = ws_reserve(ctx, &ctx->mw->ransac_ws, &ctx->mw->ransac_ws_bytes, pnp_host_ws_layout(nullptr, n, iters, &w));
    if (rc) return rc;
    pnp_host_ws_layout(ctx->mw->ransac_ws, n, iters, &w);
    StageTimer t(ctx, VO_T_POSE);
    rc = xfer_h2d(ctx, w.X, pts3d, (size_t)n * 12);
    if (!rc) rc = xfer_h2d(ctx, w.uv, pts2d, (size_t)n * 8);
    if (rc) return rc;
    const K4 K{ K4v[0], K4v[1], K4v[2], K4v[3] };
    const float thr2 = thr * thr;
    hipLaunchKernelGGL(k_pnp_hyp, dim3(div_up(iters, 64)), dim3(64), 0, ctx->stream, w.X, w.uv, n, K, iters, seed, w.Rt, w.P, nullptr);
    hipLaunchKernelGGL(k_pnp_score, dim3(div_up(iters, 4)), dim3(256), 0, ctx->stream, w.X, w.uv, n, w.P, iters, thr2, w.counts, nullptr);
    hipLaunchKernelGGL(k_ransac_best, dim3(1), dim3(1024), 0, ctx->stream, w.counts, iters, w.best);
    hipLaunchKernelGGL(k_pnp_mask, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w.X, w.uv, n, w.P, w.best, thr2, w.mask);
    VO_CHECK_LAUNCH(ctx);
    VO_HIP(ctx, hipMemcpyAsync(ctx->pinned, w.best, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_out && (rc = xfer_d2h(ctx, mask_out, w.mask, (size_t)n))) return rc;
    if (counts_out && (rc = xfer_d2h(ctx, counts_out, w.counts, (size_t)iters * 4))) return rc;
    if ((rc = xfer_flush(ctx))) return rc;
    best2_out[0] = ((int32_t*)ctx->pinned)[0];
    best2_out[1] = ((int32_t*)ctx->pinned)[1];
    VO_HIP(ctx, hipMemcpy(Rt12_out, w.Rt + (size_t)best2_out[0] * 12, 96, hipMemcpyDeviceToHost));
    return VO_OK;
}

// =========================================================================================
// Stereo PnP pair step (vo_pnp_pair / _begin / _end; no openVO counterpart): the keypoints, descriptors and disparity two slots
// already hold -> kNN-2 -> k_pnp_prep (ratio test, 3-D lookup in slot a, compaction of the usable correspondences) -> k_pnp_hyp ->
// k_pnp_score -> k_pnp_finish.  Five queue entries, no copy command, ONE host synchronisation; the arithmetic of
// vo_point_clouds -> host filter -> vo_ransac_pnp value for value (the count n stays on the device: the kernels are launched
// for the upper bound and read it), plus an optional refinement of the winner on its inliers.
// =========================================================================================

#include "pn_solve.h"

// One Gauss-Newton step of the refit by the whole block (256 threads): every thread sums its points of `mask` (i = thread + 256 k,
// ascending) into the 21 + 6 sums of J^T J and J^T r, a DPP tree sums the wave, thread 0 adds the four waves' values from LDS in
// wave order, solves and updates s_pose, or sets *s_status = -1 and leaves s_pose alone.  Ends behind a barrier: every thread may
// read s_pose and *s_status.  Shared by both forms of k_pnp_finish.
__device__ __forceinline__ void pn_gn_step(double* s_pose, double (*s_red)[27], int* s_status, const float* __restrict__ X,
                                           const float* __restrict__ uv, const uint8_t* mask, int live, const K4& K)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double R[12], acc[27];
#pragma unroll
    for (int k = 0; k < 12; k++) R[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0;
    for (int i = threadIdx.x; i < live; i += blockDim.x) {
        if (!mask[i]) continue;
        const double x = (double)X[3 * i], y = (double)X[3 * i + 1], z = (double)X[3 * i + 2];
        const double xc = ((R[0] * x + R[1] * y) + R[2] * z) + R[3];
        const double yc = ((R[4] * x + R[5] * y) + R[6] * z) + R[7];
        const double zc = ((R[8] * x + R[9] * y) + R[10] * z) + R[11];
        const double iz = 1.0 / zc;
        const double r[2] = { (K.fx * xc * iz + K.cx) - (double)uv[2 * i], (K.fy * yc * iz + K.cy) - (double)uv[2 * i + 1] };
        const double a[2][3] = { { K.fx * iz, 0.0, -K.fx * xc * iz * iz }, { 0.0, K.fy * iz, -K.fy * yc * iz * iz } };
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const double j[6] = { a[e][2] * yc - a[e][1] * zc, a[e][0] * zc - a[e][2] * xc, a[e][1] * xc - a[e][0] * yc,
                                  a[e][0], a[e][1], a[e][2] };
#pragma unroll
            for (int u = 0, k = 0; u < 6; u++)
#pragma unroll
                for (int v = u; v < 6; v++, k++) acc[k] += j[u] * j[v];
#pragma unroll
            for (int u = 0; u < 6; u++) acc[21 + u] += j[u] * r[e];
        }
    }
#pragma unroll
    for (int k = 0; k < 27; k++) {
        const double sum = wave_sum_f64_dpp(acc[k]);
        if (lane == 0) s_red[wv][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double H[21], g[6], d[6] = { 0, 0, 0, 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < 27; k++) {
            const double sum = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
            if (k < 21) H[k] = sum; else g[k - 21] = sum;
        }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 21; k++) ok = ok && isfinite(H[k]);
#pragma unroll
        for (int k = 0; k < 6; k++) ok = ok && isfinite(g[k]);
        ok = ok && pn_solve6(H, g, d);
        double Rn[12];
        for (int k = 0; k < 12; k++) Rn[k] = s_pose[k];
        if (ok) pn_apply_twist(Rn, d);
        for (int k = 0; k < 12; k++) ok = ok && isfinite(Rn[k]);
        if (ok) for (int k = 0; k < 12; k++) s_pose[k] = Rn[k];
        else *s_status = -1;
    }
    __syncthreads();
}

// The end of the step in ONE block of four waves: argmax of the inlier counts (rs_block_argmax) -> the winner's mask ->
// refine_iters Gauss-Newton steps in float64 on the winner's inliers: residual
// (fx X'/Z' + cx - u, fy Y'/Z' + cy - v), X' = R X + t, d X' / d (w, v) = [-[X']x | I]; the sums of a step are taken in a fixed
// order (pn_gn_step), so the result is a function of the inputs alone; no early exit -> the whole
// record (and the mask / q / t arrays when `arr` is given) written straight into pinned host memory.
// LO (vo_pnp_pair_lo, lo_rounds >= 1): the refit becomes lo_rounds rounds of {refine_iters steps on the present set, re-selection
// of the set under the refitted pose by the scoring kernels' own float32 test}; a round that cannot run -- fewer than 6 points in
// its set, a pivot that is not positive, a value that is not finite -- is discarded whole and ends the loop.  The record carries
// the pose and the mask arrays the set of the last completed round; see include/vo355.h.
template <bool LO>
__global__ void __launch_bounds__(256) k_pnp_finish(const int32_t* __restrict__ counts, int iters, const double* __restrict__ Rt_all,
                                                    const float* __restrict__ P_all, const float* __restrict__ X, const float* __restrict__ uv,
                                                    int nq, const int32_t* __restrict__ hdr, const int32_t* __restrict__ q2,
                                                    const int32_t* __restrict__ t2, float thr2, K4 K, int refine_iters, int lo_rounds,
                                                    uint8_t* __restrict__ mask, PnpRec* __restrict__ rec, uint8_t* __restrict__ arr, size_t cap,
                                                    PnpRec* __restrict__ rec_dev)
{
    // rec_dev (may be NULL): device memory that receives the record too, for a kernel that follows on the stream (vo_track_map)
    __shared__ long long s_key[4];
    __shared__ int s_status;
    __shared__ double s_pose[12], s_red[4][27];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_status = 1;
    int best, best_count;
    rs_block_argmax(counts, iters, s_key, best, best_count);
    const ReprojModel md{ X, uv };
    const int n = hdr[1], live = md.live(n);
    if (threadIdx.x < 12) s_pose[threadIdx.x] = Rt_all[(size_t)best * 12 + threadIdx.x];
    float P[12];
    rs_winner_model<ReprojModel>(P_all, best, P);
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        const uint8_t in = rs_inlier_of(md, P, i, live, thr2) ? 1 : 0;
        mask[i] = in;                       // (read back below by the thread that wrote it)
        if (arr) {
            arr[i] = in;
            ((int32_t*)(arr + cap))[i] = i < n ? q2[i] : -1;
            ((int32_t*)(arr + cap * 5))[i] = i < n ? t2[i] : -1;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rec->M = hdr[0]; rec->n = n; rec->best_iter = best; rec->best_count = best_count; rec->flags = hdr[2]; rec->pad = 0;
        for (int k = 0; k < 12; k++) rec->Rt[k] = s_pose[k];
        if (rec_dev) {
            rec_dev->M = hdr[0]; rec_dev->n = n; rec_dev->best_iter = best; rec_dev->best_count = best_count; rec_dev->flags = hdr[2]; rec_dev->pad = 0;
            for (int k = 0; k < 12; k++) rec_dev->Rt[k] = s_pose[k];
        }
    }
    const bool refine = refine_iters > 0 && best_count >= 6;
    int steps = 0, done = 0, support = best_count;
    if (!LO) {
        if (refine) {
            if (threadIdx.x == 0) s_status = 0;
            for (; steps < refine_iters; steps++) {
                pn_gn_step(s_pose, s_red, &s_status, X, uv, mask, live, K);
                if (s_status < 0) break;
            }
        }
    } else if (refine) {
        __shared__ double s_prev[12];
        __shared__ float s_P[12];
        __shared__ int s_cnt[4];
        int round_status = 0;                   // (uniform: what s_status would read, kept in a register between the barriers)
        for (; done < lo_rounds && support >= 6; done++) {
            if (threadIdx.x < 12) s_prev[threadIdx.x] = s_pose[threadIdx.x];
            if (threadIdx.x == 0) s_status = 0;
            __syncthreads();
            for (int k = 0; k < refine_iters; k++) {
                pn_gn_step(s_pose, s_red, &s_status, X, uv, mask, live, K);
                if (s_status < 0) break;
            }
            round_status = s_status;
            if (round_status < 0) {             // the round is discarded: the pose of the round before, the set untouched
                __syncthreads();
                if (threadIdx.x < 12) s_pose[threadIdx.x] = s_prev[threadIdx.x];
                break;
            }
            if (threadIdx.x < 4) pnp_project_col(K, s_pose, threadIdx.x, s_P);      // one column a thread
            __syncthreads();
            for (int k = 0; k < 12; k++) P[k] = s_P[k];
            int cnt = 0;
            for (int i0 = 0; i0 < nq; i0 += blockDim.x) {       // (uniform trip count: every lane takes part in the ballot)
                const int i = i0 + threadIdx.x;
                const bool in = rs_inlier_of(md, P, i, live, thr2);
                if (i < nq) mask[i] = in ? 1 : 0;              // (its own points: read back by the thread that wrote them)
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) s_cnt[wv] = cnt;
            __syncthreads();
            support = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
            steps += refine_iters;
        }
        __syncthreads();
        // status: 0 once a round is complete; otherwise round 1's, which is the plain refit's for the same inputs
        if (threadIdx.x == 0) s_status = done >= 1 ? 0 : (round_status < 0 ? -1 : 1);
        if (arr && done >= 1)
            for (int i = threadIdx.x; i < nq; i += blockDim.x) arr[i] = mask[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rec->rstatus = s_status; rec->rsteps = steps;
        for (int k = 0; k < 12; k++) rec->Rtr[k] = s_pose[k];
        if (LO) { rec->lo_rounds = done; rec->lo_support = support; }
        if (rec_dev) {
            rec_dev->rstatus = s_status; rec_dev->rsteps = steps;
            for (int k = 0; k < 12; k++) rec_dev->Rtr[k] = s_pose[k];
            if (LO) { rec_dev->lo_rounds = done; rec_dev->lo_support = support; }
        }
    }
}

int pnp_ranges_check(vo_ctx* ctx, const double* K4v, int iters, float thr, int refine_iters, const char* who)
{
    if (iters <= 0 || iters > (1 << 22)) return vo_fail(ctx, VO_E_ARG, "%s: need 0 < iters <= 4194304", who);
    if (refine_iters < 0 || refine_iters > 20) return vo_fail(ctx, VO_E_ARG, "%s: refine_iters is 0 .. 20", who);
    if (!(thr > 0.0f) || !(K4v[0] > 0.0) || !(K4v[1] > 0.0)) return vo_fail(ctx, VO_E_ARG, "%s: need thr > 0 and positive focal lengths", who);
    return VO_OK;
}

// lg: the loop gate of the step, as the context stands at this call (a ticket keeps it)
int pnp_check(vo_ctx* ctx, int slot_a, int slot_b, int match_flags, const double* K4v, int iters, float thr, int refine_iters, const char* who,
              LoopGate* lg, int view_n)
{
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !K4v)
        return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (int rcf = match_flags_check(ctx, match_flags, who, true)) return rcf;
    if (int rcr = pnp_ranges_check(ctx, K4v, iters, thr, refine_iters, who)) return rcr;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (view_n >= 0) {                       // slot a will be a view: depth-carrying keypoints, view_n of them
        if (!slot_sparse(b)) return vo_fail(ctx, VO_E_STATE, "%s: slot %d: the keypoints carry no depth (vo_sparse_stereo)", who, slot_b);
        if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
        if (view_n > 0 && b.n_kp < 2) return vo_fail(ctx, VO_E_ARG, "train set has fewer than 2 descriptors");
        *lg = LoopGate();
        if (match_flags & VO_MATCH_LOOP) { lg->rd_a = a.kp_rdesc; lg->rd_b = b.kp_rdesc; lg->max_h = ctx->loop_max; }
        return VO_OK;
    }
    if (!a.has_kp || !b.has_kp) return vo_fail(ctx, VO_E_STATE, "%s: both slots need disparity and keypoints", who);
    if (slot_sparse(a) != slot_sparse(b)) return vo_fail(ctx, VO_E_STATE, "%s: one slot's keypoints carry depth, the other's do not", who);
    if (!slot_sparse(a) && (!a.has_disp || !b.has_disp)) return vo_fail(ctx, VO_E_STATE, "%s: both slots need disparity and keypoints", who);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    if (a.n_kp > 0 && b.n_kp < 2) return vo_fail(ctx, VO_E_ARG, "train set has fewer than 2 descriptors");
    return match_loop_gate(ctx, a, b, match_flags, who, lg);
}

// the RANSAC workspace of the match scratch currently installed in ctx (the main one, or a pose alternate's), laid out for one step
int pnp_ws_take(vo_ctx* ctx, int nq, int iters, PnpWs* ws)
{
    // the floor (256 hypotheses on kp_cap keypoints) makes the first allocation the last one on the steady path
    const size_t need = pnp_ws_layout(nullptr, nq, iters, ws), floor = pnp_ws_layout(nullptr, ctx->kp_cap, 256, ws);
    if (int rc = ws_reserve(ctx, &ctx->mw->ransac_ws, &ctx->mw->ransac_ws_bytes, need, floor)) return rc;
    pnp_ws_layout(ctx->mw->ransac_ws, nq, iters, ws);
    return VO_OK;
}

// everything behind the prep launch: hypotheses, scores and the finish on ctx->stream, for the upper bound nq (the kernels read n)
int pnp_tail_enqueue(vo_ctx* ctx, const PnpWs& w, int nq, const double* K4v, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds,
                     PnpRec* rec, uint8_t* arr, PnpRec* rec_dev)
{
    const PnpDev& d = w.d;
    const K4 K{ K4v[0], K4v[1], K4v[2], K4v[3] };
    const float thr2 = thr * thr;
    hipLaunchKernelGGL(k_pnp_hyp, dim3(div_up(iters, 64)), dim3(64), 0, ctx->stream, d.X, d.uv, nq, K, iters, seed, w.Rt, w.P, d.hdr + 1);
    hipLaunchKernelGGL(k_pnp_score, dim3(div_up(iters, 4)), dim3(256), 0, ctx->stream, d.X, d.uv, nq, w.P, iters, thr2, w.counts, d.hdr + 1);
    // (the plain form is launched whenever no round is asked for: the LO entries with lo_rounds == 0 ARE the plain entries)
    auto finish = lo_rounds > 0 ? k_pnp_finish<true> : k_pnp_finish<false>;
    hipLaunchKernelGGL(finish, dim3(1), dim3(256), 0, ctx->stream, w.counts, iters, w.Rt, w.P, d.X, d.uv, nq, d.hdr, d.q, d.t, thr2, K,
                       refine_iters, lo_rounds, w.mask, rec, arr, pnp_cap(ctx->kp_cap), rec_dev);
    VO_CHECK_LAUNCH(ctx);
    return VO_OK;
}

// the whole chain on ctx->stream with the match scratch and RANSAC workspace currently installed in ctx (the main ones, or a
// pose alternate's); rec / arr: pinned host memory k_pnp_finish writes (arr may be NULL)
int pnp_enqueue(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, double ratio, int match_flags, const double* K4v, int iters, float thr, uint32_t seed,
                int refine_iters, PnpRec* rec, uint8_t* arr, const LoopGate& lg, PnpChain* chain, int lo_rounds)
{
    const int nq = a.n_kp, cross = match_flags & VO_MATCH_CROSSCHECK;
    PnpWs w;
    int rc;
    if ((rc = pnp_ws_take(ctx, nq, iters, &w))) return rc;
    {
        StageTimer t(ctx, VO_T_MATCH);
        if ((rc = match_knn2_slots(ctx, a, b, match_flags))) return rc;
    }
    {
        StageTimer t(ctx, VO_T_POSE);
        if ((rc = pnp_prep_launch(ctx, a, b, ratio, cross, w.d, lg, chain ? chain->nq_dev : nullptr))) return rc;
        if ((rc = pnp_tail_enqueue(ctx, w, nq, K4v, iters, thr, seed, refine_iters, lo_rounds, rec, arr, chain ? chain->rec_dev : nullptr))) return rc;
    }
    if (chain) { chain->d = w.d; chain->mask = w.mask; }
    return VO_OK;
}

void pnp_rec_clear(PnpRec* r)
{
    memset(r, 0, sizeof(PnpRec));
    r->rstatus = 1;
}

// record (+ arrays) -> the caller's outputs; VO_E_STATE for a pair the step refused.  lo2 (may be NULL) = {rounds completed, |S_c|}
int pnp_unpack(vo_ctx* ctx, const PnpRec* r, const uint8_t* arr, int nq, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
               int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, const char* who, int lo_rounds, int32_t* lo2)
{
    counts4[0] = r->M; counts4[1] = r->n; counts4[2] = r->best_iter; counts4[3] = r->best_count;
    *flags = r->flags;
    memcpy(Rt12, r->Rt, sizeof(r->Rt));
    refine2[0] = r->rstatus; refine2[1] = r->rsteps;
    if (lo2) { lo2[0] = lo_rounds > 0 ? r->lo_rounds : 0; lo2[1] = lo_rounds > 0 ? r->lo_support : r->best_count; }
    if (Rt12_refined) memcpy(Rt12_refined, r->Rtr, sizeof(r->Rtr));
    if (arr) {
        const size_t cap = pnp_cap(ctx->kp_cap);
        if (mask_out) memcpy(mask_out, arr, (size_t)nq);
        if (q_idx) memcpy(q_idx, arr + cap, (size_t)nq * 4);
        if (t_idx) memcpy(t_idx, arr + cap * 5, (size_t)nq * 4);
    }
    if (r->flags & 2) return vo_fail(ctx, VO_E_STATE, "%s: a match index lies outside the train set: the pair is refused", who);
    return VO_OK;
}

int pnp_lo_check(vo_ctx* ctx, int lo_rounds, int refine_iters, const char* who)
{
    if (!ctx) return VO_E_ARG;
    if (lo_rounds < 0 || lo_rounds > 8) return vo_fail(ctx, VO_E_ARG, "%s: lo_rounds is 0 .. 8", who);
    if (lo_rounds > 0 && refine_iters < 1) return vo_fail(ctx, VO_E_ARG, "%s: lo_rounds >= 1 needs refine_iters >= 1", who);
    return VO_OK;
}

static int pnp_pair_impl(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                         uint32_t seed, int refine_iters, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
                         int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds, int32_t* lo2, const char* who)
{
    if (ctx && (!counts4 || !flags || !Rt12 || !refine2)) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    LoopGate lg;
    int rc = pnp_check(ctx, slot_a, slot_b, match_flags, K4v, iters, thr, refine_iters, who, &lg);
    if (rc) return rc;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    const bool want = mask_out || q_idx || t_idx;
    if (want && cap < a.n_kp) return vo_fail(ctx, VO_E_CAP, "%s: outputs hold %d entries, %d keypoints", who, cap, a.n_kp);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    PnpRec* rec = (PnpRec*)ctx->pinned;
    pnp_rec_clear(rec);
    uint8_t* arr = nullptr;
    if (a.n_kp > 0) {
        const size_t bytes = pnp_cap(ctx->kp_cap) * 9;
        if (want && !(arr = (uint8_t*)xfer_stage(ctx, bytes))) {
            if ((rc = xfer_flush(ctx))) return rc;
            if (!(arr = (uint8_t*)xfer_stage(ctx, bytes))) return vo_fail(ctx, VO_E_CAP, "%s: the transfer arena cannot hold %d keypoints", who, a.n_kp);
        }
        if ((rc = pnp_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, rec, arr, lg, nullptr, lo_rounds))) return rc;
        if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
        if (!slot_sparse(a) && ((rc = slot_health(ctx, a, slot_a)) || (rc = slot_health(ctx, b, slot_b)))) return rc;   // never a pose from an undefined disparity
    }
    return pnp_unpack(ctx, rec, arr, a.n_kp, counts4, flags, Rt12, Rt12_refined, refine2, mask_out, q_idx, t_idx, who, lo_rounds, lo2);
}

extern "C" int vo_pnp_pair(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                           uint32_t seed, int refine_iters, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
                           int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap)
{
    return pnp_pair_impl(ctx, slot_a, slot_b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, counts4, flags, Rt12, Rt12_refined, refine2,
                         mask_out, q_idx, t_idx, cap, 0, nullptr, "vo_pnp_pair");
}

extern "C" int vo_pnp_pair_lo(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                              uint32_t seed, int refine_iters, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined,
                              int32_t* refine2, uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int lo_rounds, int32_t* lo2)
{
    if (ctx && !lo2) return vo_fail(ctx, VO_E_ARG, "vo_pnp_pair_lo: bad argument");
    if (int rc = pnp_lo_check(ctx, lo_rounds, refine_iters, "vo_pnp_pair_lo")) return rc;
    return pnp_pair_impl(ctx, slot_a, slot_b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, counts4, flags, Rt12, Rt12_refined, refine2,
                         mask_out, q_idx, t_idx, cap, lo_rounds, lo2, "vo_pnp_pair_lo");
}

// The same step in two halves on a POSE alternate (vo_ctx::ALT_POSE: the tickets, streams and scratch of vo_pose_pair_begin --
// VO_NUM_POSE_ASYNC bounds both kinds together, no stream is added)
static int pnp_begin_impl(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                          uint32_t seed, int refine_iters, int want_matches, int lo_rounds, int* ticket_out, const char* who)
{
    if (ctx && !ticket_out) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    LoopGate lg;
    int rc = pnp_check(ctx, slot_a, slot_b, match_flags, K4v, iters, thr, refine_iters, who, &lg);
    if (rc) return rc;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    int k;
    if ((rc = alt_open(ctx, vo_ctx::ALT_POSE, a, b, who, &k))) return rc;
    vo_ctx::PoseAlt& p = ctx->pose_alt[k];
    pnp_rec_clear((PnpRec*)p.result);
    if (a.n_kp > 0) {
        AltScope on_alt(ctx, p);
        rc = pnp_enqueue(ctx, a, b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, (PnpRec*)p.result,
                         want_matches ? p.result + PNP_HDR : nullptr, lg, nullptr, lo_rounds);
    }
    if (rc) return rc;
    p.slot_a = slot_a; p.slot_b = slot_b;
    p.gen_a = a.disp_gen; p.gen_b = b.disp_gen;
    if (slot_sparse(a)) p.gen_a = p.gen_b = 0;       // the step read no disparity: nothing to check at _end
    p.pnp = true; p.klt = false; p.want = want_matches != 0 && a.n_kp > 0; p.nq = a.n_kp; p.lo = lo_rounds;
    return alt_close(ctx, vo_ctx::ALT_POSE, k, a, b, ticket_out);
}

extern "C" int vo_pnp_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                                 uint32_t seed, int refine_iters, int want_matches, int* ticket_out)
{
    return pnp_begin_impl(ctx, slot_a, slot_b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, want_matches, 0, ticket_out, "vo_pnp_pair_begin");
}

extern "C" int vo_pnp_pair_begin_lo(vo_ctx* ctx, int slot_a, int slot_b, double ratio, int match_flags, const double* K4v, int iters, float thr,
                                    uint32_t seed, int refine_iters, int want_matches, int lo_rounds, int* ticket_out)
{
    if (int rc = pnp_lo_check(ctx, lo_rounds, refine_iters, "vo_pnp_pair_begin_lo")) return rc;
    return pnp_begin_impl(ctx, slot_a, slot_b, ratio, match_flags, K4v, iters, thr, seed, refine_iters, want_matches, lo_rounds, ticket_out,
                          "vo_pnp_pair_begin_lo");
}

// either _end ends a PnP ticket of either kind (the rounds are the ticket's); the plain one returns no lo2
static int pnp_end_impl(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                        uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int32_t* lo2, const char* who)
{
    int rc = alt_ticket(ctx, vo_ctx::ALT_POSE, ticket, counts4 && flags && Rt12 && refine2, who);
    if (rc) return rc;
    vo_ctx::PoseAlt& p = ctx->pose_alt[ticket];
    if (!p.pnp) return vo_fail(ctx, VO_E_STATE, "%s: ticket %d belongs to vo_pose_pair_begin (end it with vo_pose_pair_end)", who, ticket);
    if (p.klt) return vo_fail(ctx, VO_E_STATE, "%s: ticket %d belongs to vo_klt_pnp_pair_begin (end it with vo_klt_pnp_pair_end)", who, ticket);
    if ((mask_out || q_idx || t_idx) && p.nq > 0 && (!p.want || cap < p.nq))
        return vo_fail(ctx, VO_E_CAP, "%s: outputs hold %d entries, %d keypoints (or the step was begun without want_matches)", who, cap, p.nq);
    if ((rc = alt_wait(ctx, p))) return rc;
    const int32_t gens[2] = { p.gen_a, p.gen_b };
    const int slots[2] = { p.slot_a, p.slot_b };
    for (int i = 0; i < 2; i++) {
        const FrameSlot& f = ctx->slots[slots[i]];
        if (gens[i] != 0 && *(volatile int32_t*)f.sweep_word == gens[i])
            return vo_fail(ctx, VO_E_SWEEP, "PnP step %d: the aggregation sweep of the pair in slot %d gave up a strip hand-off: its "
                                            "disparity is undefined and no pose is derived from it", ticket, slots[i]);
    }
    return pnp_unpack(ctx, (const PnpRec*)p.result, p.want ? p.result + PNP_HDR : nullptr, p.nq, counts4, flags, Rt12, Rt12_refined, refine2,
                      mask_out, q_idx, t_idx, who, p.lo, lo2);
}

extern "C" int vo_pnp_pair_end(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                               uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap)
{
    return pnp_end_impl(ctx, ticket, counts4, flags, Rt12, Rt12_refined, refine2, mask_out, q_idx, t_idx, cap, nullptr, "vo_pnp_pair_end");
}

extern "C" int vo_pnp_pair_end_lo(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                                  uint8_t* mask_out, int32_t* q_idx, int32_t* t_idx, int cap, int32_t* lo2)
{
    return pnp_end_impl(ctx, ticket, counts4, flags, Rt12, Rt12_refined, refine2, mask_out, q_idx, t_idx, cap, lo2, "vo_pnp_pair_end_lo");
}
