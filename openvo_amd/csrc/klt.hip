// Pyramidal Lucas-Kanade tracking with a forward-backward check (include/vo355.h, vo_klt_*): NOT part of the reference, defined by
// this build operation by operation; tests/klt_ref.py restates it and the kernels below are held to it bit for bit.
//   k_klt_pyr_down   one pyramid level of BOTH images per launch ([1 4 6 4 1] separable, reflected borders, integer exact)
//   k_klt_track      one wave per point, VO_KLT_WAVES points per workgroup: the win x win window over the 64 lanes, the template
//                    (I, Dx, Dy of image A) in registers as packed int16 for a whole level, per iteration a gather of the four taps
//                    of J from the level image of B, int32 partial sums per lane, an int64 butterfly over the wave (integer sums are
//                    order-free) and the scalar float64 step computed by every lane alike.  Nothing is handed between waves: no LDS,
//                    no atomics, no counters, no waiting; every loop is bounded by levels, iters and the window; every read is clamped.
// and the host side of vo_klt_pnp_pair / _begin / _end at the end of the file: the two kernels above, k_klt_pnp_prep (geom.hip) and the
// tail of the stereo PnP step (ransac.hip) as one chain.
#include <math.h>
#include "vo_internal.h"

#define VO_KLT_WAVES 4

struct KltImgs {
    const uint8_t* a[VO_KLT_MAX_LEVELS];
    const uint8_t* b[VO_KLT_MAX_LEVELS];
    int w[VO_KLT_MAX_LEVELS], h[VO_KLT_MAX_LEVELS];
};
struct KltPrm {
    int win, levels, iters, magic;      // magic = ceil(65536 / win): p / win == (p * magic) >> 16 for p < 1024, win <= 31
    double eps2, min_eig, fb2, ox, oy;  // eps eps, fb fb (rounded products of the host's doubles), the origin
};

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int klt_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// 32 x 8 outputs per workgroup from a 67 x 19 source tile; blockIdx.z = image
__global__ void __launch_bounds__(256) k_klt_pyr_down(const uint8_t* __restrict__ srcA, const uint8_t* __restrict__ srcB, uint8_t* __restrict__ dstA,
                                                      uint8_t* __restrict__ dstB, int w, int h, int ow, int oh)
{
    __shared__ uint8_t s_src[19][68];
    __shared__ uint16_t s_h[19][32];
    const uint8_t* __restrict__ src = blockIdx.z ? srcB : srcA;
    uint8_t* __restrict__ dst = blockIdx.z ? dstB : dstA;
    const int tid = threadIdx.y * 32 + threadIdx.x;
    const int x0 = 2 * (int)blockIdx.x * 32 - 2, y0 = 2 * (int)blockIdx.y * 8 - 2;
    for (int k = tid; k < 19 * 67; k += 256) {
        const int r = k / 67, c = k - r * 67;
        s_src[r][c] = src[(size_t)klt_reflect(y0 + r, h) * w + klt_reflect(x0 + c, w)];
    }
    __syncthreads();
    for (int k = tid; k < 19 * 32; k += 256) {
        const int r = k >> 5, x = k & 31;
        const uint8_t* p = &s_src[r][2 * x];
        s_h[r][x] = (uint16_t)(p[0] + 4 * p[1] + 6 * p[2] + 4 * p[3] + p[4]);
    }
    __syncthreads();
    const int ox = blockIdx.x * 32 + threadIdx.x, oy = blockIdx.y * 8 + threadIdx.y;
    if (ox < ow && oy < oh) {
        const int ty = 2 * threadIdx.y, tx = threadIdx.x;
        const int v = s_h[ty][tx] + 4 * s_h[ty + 1][tx] + 6 * s_h[ty + 2][tx] + 4 * s_h[ty + 3][tx] + s_h[ty + 4][tx];
        dst[(size_t)oy * ow + ox] = (uint8_t)((v + 128) >> 8);
    }
}

// ---- tracking --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int klt_rd(const uint8_t* __restrict__ img, int w, int h, int x, int y)
{
    x = min(max(x, 0), w - 1);
    y = min(max(y, 0), h - 1);
    return img[(size_t)y * w + x];
}

struct KltCorner { int ix, iy, w00, w01, w10, w11; };
__device__ __forceinline__ KltCorner klt_corner(double cx, double cy, double half)
{
    const double tx = cx - half, ty = cy - half;
    const double flx = floor(tx), fly = floor(ty);
    const double fx = tx - flx, fy = ty - fly;
    KltCorner c;
    c.ix = (int)fmin(fmax(flx, -1073741824.0), 1073741824.0);
    c.iy = (int)fmin(fmax(fly, -1073741824.0), 1073741824.0);
    c.w00 = (int)rint(((1.0 - fx) * (1.0 - fy)) * 16384.0);
    c.w01 = (int)rint((fx * (1.0 - fy)) * 16384.0);
    c.w10 = (int)rint(((1.0 - fx) * fy) * 16384.0);
    c.w11 = 16384 - c.w00 - c.w01 - c.w10;
    return c;
}

__device__ __forceinline__ long long klt_wave_sum(int v)
{
    long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// -1 for a window pixel p < npx, 0 past the window: a sign mask in a vector register.  The empty asm keeps the compiler from turning
// it back into a compare whose lane mask it then keeps in a scalar register pair per trip: sixteen of those do not fit.
__device__ __forceinline__ int klt_inside(int p, int npx)
{
    int m = (p - npx) >> 31;
    asm("" : "+v"(m));
    return m;
}

// one direction of one point, by one wave: from image A's pyramid into B's (swap: from B's into A's), starting at the finite
// position (p0x, p0y) in level-0 pixels; every lane returns the same q, status and count
template <int TRIPS>
__device__ __forceinline__ void klt_run(const KltImgs& P, const KltPrm& prm, bool swap, double p0x, double p0y, int lane, double& qx, double& qy,
                                        int& status, int& count)
{
    const int win = prm.win, npx = win * win;
    const double half = (double)((win - 1) / 2), dwin = (double)win;
    // window pixel of this lane in trip t: u | v << 8.  A lane past the window works on pixel (0, 0) with a zero template: its
    // products vanish, and no mask has to stay live across the iterations.
    int pu[TRIPS];
#pragma unroll
    for (int t = 0; t < TRIPS; t++) {
        const int p = t * 64 + lane, v = (p * prm.magic) >> 16;
        pu[t] = ((p - v * win) | (v << 8)) & klt_inside(p, npx);
    }
    const double top = 1.0 / (double)(1 << (prm.levels - 1));
    qx = p0x * top; qy = p0y * top;
    status = 0; count = 0;
    bool dead = false;
    for (int L = prm.levels - 1; L >= 0 && !dead; --L) {
        const uint8_t* __restrict__ A = swap ? P.b[L] : P.a[L];
        const uint8_t* __restrict__ B = swap ? P.a[L] : P.b[L];
        const int wL = P.w[L], hL = P.h[L];
        const double sc = 1.0 / (double)(1 << L);
        // template: I (5 fractional bits) | Dx << 16, and Dy two to a word
        int tA[TRIPS], tB[(TRIPS + 1) / 2];
        int a11 = 0, a12 = 0, a22 = 0;
        {
            const KltCorner c = klt_corner(p0x * sc, p0y * sc, half);
#pragma unroll
            for (int t = 0; t < TRIPS; t++) {
                int I, dx, dy;
                {
                    const int x = c.ix + (pu[t] & 255), y = c.iy + (pu[t] >> 8);
                    int v[4][4];
#pragma unroll
                    for (int r = 0; r < 4; r++)
#pragma unroll
                        for (int k = 0; k < 4; k++) v[r][k] = klt_rd(A, wL, hL, x - 1 + k, y - 1 + r);
                    int gx[2][2], gy[2][2];
#pragma unroll
                    for (int b = 0; b < 2; b++)
#pragma unroll
                        for (int a = 0; a < 2; a++) {
                            gx[b][a] = 3 * (v[b][a + 2] - v[b][a]) + 10 * (v[b + 1][a + 2] - v[b + 1][a]) + 3 * (v[b + 2][a + 2] - v[b + 2][a]);
                            gy[b][a] = 3 * (v[b + 2][a] - v[b][a]) + 10 * (v[b + 2][a + 1] - v[b][a + 1]) + 3 * (v[b + 2][a + 2] - v[b][a + 2]);
                        }
                    I = (c.w00 * v[1][1] + c.w01 * v[1][2] + c.w10 * v[2][1] + c.w11 * v[2][2] + 256) >> 9;
                    dx = (c.w00 * gx[0][0] + c.w01 * gx[0][1] + c.w10 * gx[1][0] + c.w11 * gx[1][1] + 8192) >> 14;
                    dy = (c.w00 * gy[0][0] + c.w01 * gy[0][1] + c.w10 * gy[1][0] + c.w11 * gy[1][1] + 8192) >> 14;
                }
                { const int m = klt_inside(t * 64 + lane, npx); I &= m; dx &= m; dy &= m; }
                tA[t] = (I & 0xffff) | (int)((unsigned)dx << 16);
                if (t & 1) tB[t >> 1] |= (int)((unsigned)dy << 16);
                else tB[t >> 1] = dy & 0xffff;
                a11 += dx * dx; a12 += dx * dy; a22 += dy * dy;
            }
        }
        const double A11 = (double)klt_wave_sum(a11), A12 = (double)klt_wave_sum(a12), A22 = (double)klt_wave_sum(a22);
        const double D = A11 * A22 - A12 * A12;
        const double s = 9.5367431640625e-07;        // 2^-20
        const double me = ((A22 + A11) * s - sqrt(((A11 - A22) * s) * ((A11 - A22) * s) + (4.0 * (A12 * s)) * (A12 * s))) / (double)(2 * win * win);
        if (me < prm.min_eig || D <= 0.0) {
            if (L == 0) status |= 1;
        } else {
            double dxp = 0.0, dyp = 0.0;
            for (int k = 0; k < prm.iters; k++) {
                if (!(qx >= -dwin && qx <= (double)(wL - 1) + dwin && qy >= -dwin && qy <= (double)(hL - 1) + dwin)) {
                    const double up = (double)(1 << L);
                    status |= 2; dead = true;
                    qx = qx * up; qy = qy * up;
                    break;
                }
                count++;
                const KltCorner c = klt_corner(qx, qy, half);
                int b1 = 0, b2 = 0;
#pragma unroll
                for (int t = 0; t < TRIPS; t++) {
                        const int x = c.ix + (pu[t] & 255), y = c.iy + (pu[t] >> 8);
                        const int i00 = klt_rd(B, wL, hL, x, y), i01 = klt_rd(B, wL, hL, x + 1, y);
                        const int i10 = klt_rd(B, wL, hL, x, y + 1), i11 = klt_rd(B, wL, hL, x + 1, y + 1);
                        const int J = (c.w00 * i00 + c.w01 * i01 + c.w10 * i10 + c.w11 * i11 + 256) >> 9;
                        const int dI = J - (int)(int16_t)(tA[t] & 0xffff);
                        const int dy = (t & 1) ? (tB[t >> 1] >> 16) : (int)(int16_t)(tB[t >> 1] & 0xffff);
                        b1 += dI * (tA[t] >> 16);
                        b2 += dI * dy;
                    }
                const double B1 = (double)klt_wave_sum(b1), B2 = (double)klt_wave_sum(b2);
                const double dx = (A12 * B2 - A22 * B1) / D, dy = (A12 * B1 - A11 * B2) / D;
                qx = qx + dx; qy = qy + dy;
                if (dx * dx + dy * dy <= prm.eps2) break;
                if (k >= 1 && fabs(dx + dxp) < 0.01 && fabs(dy + dyp) < 0.01) {
                    qx = qx - 0.5 * dx; qy = qy - 0.5 * dy;
                    break;
                }
                dxp = dx; dyp = dy;
            }
        }
        if (!dead && L > 0) { qx = qx * 2.0; qy = qy * 2.0; }
    }
    if (!dead && !(qx >= 0.0 && qx <= (double)(P.w[0] - 1) && qy >= 0.0 && qy <= (double)(P.h[0] - 1))) status |= 2;
}

// backward = 0: xy_in -> xy_out, status, iters.  backward = 1: the points with status 0 from xy_out back into image A; bit 8 and the
// iteration counts are added (xy_out stays the forward result).
template <int TRIPS>
__global__ void __launch_bounds__(64 * VO_KLT_WAVES, 2) k_klt_track(KltImgs P, KltPrm prm, const float* __restrict__ xy_in, float* xy_out, uint8_t* status,
                                                                int32_t* iters, int n, int backward)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * VO_KLT_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const float x = xy_in[2 * (size_t)i], y = xy_in[2 * (size_t)i + 1];
    double qx, qy;
    int st, cnt;
    if (!backward) {
        if (!(isfinite(x) && isfinite(y))) {
            if (lane == 0) { xy_out[2 * (size_t)i] = x; xy_out[2 * (size_t)i + 1] = y; status[i] = 4; iters[i] = 0; }
            return;
        }
        klt_run<TRIPS>(P, prm, false, (double)x + prm.ox, (double)y + prm.oy, lane, qx, qy, st, cnt);
        if (lane == 0) {
            xy_out[2 * (size_t)i] = (float)(qx - prm.ox); xy_out[2 * (size_t)i + 1] = (float)(qy - prm.oy);
            status[i] = (uint8_t)st; iters[i] = cnt;
        }
    } else {
        if (status[i] != 0) return;
        const float fx = xy_out[2 * (size_t)i], fy = xy_out[2 * (size_t)i + 1];
        klt_run<TRIPS>(P, prm, true, (double)fx + prm.ox, (double)fy + prm.oy, lane, qx, qy, st, cnt);
        const float bx = (float)(qx - prm.ox), by = (float)(qy - prm.oy);
        const double ex = (double)bx - (double)x, ey = (double)by - (double)y;
        const double d2 = ex * ex + ey * ey;
        if (lane == 0) {
            if (st != 0 || !(d2 <= prm.fb2)) status[i] = 8;
            iters[i] += cnt;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
void klt_ws_free(KltWs& k)
{
    void* ps[] = { k.pyr[0], k.pyr[1], k.xy_in, k.xy_out, k.status, k.iters };
    for (void* p : ps) if (p) (void)hipFree(p);
    k = KltWs();
}

// completes the Lucas-Kanade members of the match workspace in force (the main one, or a pose alternate's under its AltScope)
int klt_ws_prepare(vo_ctx* ctx)
{
    KltWs& k = ctx->mw->klt;
    if (k.ready) return VO_OK;
    size_t total = 0;
    int w = ctx->max_w, h = ctx->max_h;
    for (int l = 0; l < VO_KLT_MAX_LEVELS; l++) {
        k.off[l] = total;
        total += ((size_t)w * h + 255) & ~(size_t)255;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    const size_t cap = (size_t)ctx->kp_cap;
    hipError_t e = hipMalloc((void**)&k.pyr[0], total);
    if (e == hipSuccess) e = hipMalloc((void**)&k.pyr[1], total);
    if (e == hipSuccess) e = hipMalloc((void**)&k.xy_in, cap * 8 + 256);
    if (e == hipSuccess) e = hipMalloc((void**)&k.xy_out, cap * 8 + 256);
    if (e == hipSuccess) e = hipMalloc((void**)&k.status, cap + 256);
    if (e == hipSuccess) e = hipMalloc((void**)&k.iters, cap * 4 + 256);
    if (e != hipSuccess) {
        klt_ws_free(k);
        return vo_fail(ctx, VO_E_HIP, "Lucas-Kanade workspace allocation failed: %s", hipGetErrorString(e));
    }
    k.ready = true;
    return VO_OK;
}

static int klt_params(vo_ctx* ctx, int win, int levels, int iters, double eps, double min_eig, double fb, const char* who, KltPrm* p)
{
    if (win < 5 || win > 31 || !(win & 1)) return vo_fail(ctx, VO_E_ARG, "%s: win %d (odd, 5 .. 31)", who, win);
    if (levels < 1 || levels > VO_KLT_MAX_LEVELS) return vo_fail(ctx, VO_E_ARG, "%s: levels %d (1 .. %d)", who, levels, VO_KLT_MAX_LEVELS);
    if (iters < 1 || iters > 100) return vo_fail(ctx, VO_E_ARG, "%s: iters %d (1 .. 100)", who, iters);
    if (!(isfinite(eps) && eps >= 0 && isfinite(min_eig) && min_eig >= 0 && isfinite(fb) && fb >= 0))
        return vo_fail(ctx, VO_E_ARG, "%s: eps, min_eig and fb must be finite and >= 0", who);
    p->win = win; p->levels = levels; p->iters = iters; p->magic = (65536 + win - 1) / win;
    p->eps2 = eps * eps; p->min_eig = min_eig; p->fb2 = fb * fb; p->ox = 0.0; p->oy = 0.0;
    return VO_OK;
}

// the pyramids above level 0 of both images into the Lucas-Kanade workspace of the match scratch in force (prepared by the caller:
// klt_ws_prepare), one launch per level on ctx->stream; a / b / lw / lh: VO_KLT_MAX_LEVELS entries each, level l's images and size
// (the levels from `levels` on repeat level 0: never read, always valid).  Shared with the direct alignment (direct.hip).
int klt_pyr_enqueue(vo_ctx* ctx, const uint8_t* a0, const uint8_t* b0, int w, int h, int levels, const uint8_t** a, const uint8_t** b, int* lw, int* lh)
{
    KltWs& k = ctx->mw->klt;
    for (int l = 0; l < VO_KLT_MAX_LEVELS; l++) { a[l] = a0; b[l] = b0; lw[l] = w; lh[l] = h; }     // (levels never read stay valid)
    StageTimer t(ctx, VO_T_ORB, levels > 1 ? levels - 1 : 1);
    for (int l = 1; l < levels; l++) {
        const int ow = (lw[l - 1] + 1) / 2, oh = (lh[l - 1] + 1) / 2;
        uint8_t *da = k.pyr[0] + k.off[l], *db = k.pyr[1] + k.off[l];
        hipLaunchKernelGGL(k_klt_pyr_down, dim3(div_up(ow, 32), div_up(oh, 8), 2), dim3(32, 8), 0, ctx->stream, a[l - 1], b[l - 1], da, db,
                           lw[l - 1], lh[l - 1], ow, oh);
        VO_CHECK_LAUNCH(ctx);
        a[l] = da; b[l] = db; lw[l] = ow; lh[l] = oh;
    }
    return VO_OK;
}

// the pyramids above level 0 of both images, then the forward (and backward) pass of the n points at d_xy, all on ctx->stream
static int klt_enqueue(vo_ctx* ctx, const uint8_t* a0, const uint8_t* b0, int w, int h, const KltPrm& prm, bool fb, const float* d_xy, int n)
{
    KltWs& k = ctx->mw->klt;
    KltImgs P;
    if (int rc = klt_pyr_enqueue(ctx, a0, b0, w, h, prm.levels, P.a, P.b, P.w, P.h)) return rc;
    const int trips = div_up(prm.win * prm.win, 64);
    auto kern = trips <= 2 ? k_klt_track<2> : trips <= 4 ? k_klt_track<4> : trips <= 7 ? k_klt_track<7> : trips <= 10 ? k_klt_track<10> : k_klt_track<16>;
    StageTimer t(ctx, VO_T_MATCH, fb ? 2 : 1);
    for (int back = 0; back < (fb ? 2 : 1); back++) {
        hipLaunchKernelGGL(kern, dim3(div_up(n, VO_KLT_WAVES)), dim3(64 * VO_KLT_WAVES), 0, ctx->stream, P, prm, d_xy, k.xy_out, k.status,
                           k.iters, n, back);
        VO_CHECK_LAUNCH(ctx);
    }
    return VO_OK;
}

extern "C" int vo_klt_track_host(vo_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, const float* xy, int n, int win, int levels,
                                 int iters, double eps, double min_eig, double fb, float* xy_out, uint8_t* status_out, int32_t* iters_out)
{
    if (!ctx || !img_a || !img_b || w <= 0 || h <= 0 || n < 0) return vo_fail(ctx, VO_E_ARG, "vo_klt_track_host: bad argument");
    KltPrm prm;
    if (int rc = klt_params(ctx, win, levels, iters, eps, min_eig, fb, "vo_klt_track_host", &prm)) return rc;
    if (w > ctx->max_w || h > ctx->max_h) return vo_fail(ctx, VO_E_CAP, "image %dx%d exceeds context", w, h);
    if (n > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "n=%d exceeds keypoint capacity %d", n, ctx->kp_cap);
    if (n > 0 && (!xy || !xy_out || !status_out || !iters_out)) return vo_fail(ctx, VO_E_ARG, "vo_klt_track_host: null pointer");
    if (n == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = klt_ws_prepare(ctx)) return rc;
    KltWs& k = ctx->mw->klt;
    const size_t npx = (size_t)w * h;
    VO_HIP(ctx, hipMemcpyAsync(k.pyr[0], img_a, npx, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP(ctx, hipMemcpyAsync(k.pyr[1], img_b, npx, hipMemcpyHostToDevice, ctx->stream));
    int rc = xfer_h2d(ctx, k.xy_in, xy, (size_t)n * 8);
    if (!rc) rc = klt_enqueue(ctx, k.pyr[0], k.pyr[1], w, h, prm, fb > 0, k.xy_in, n);
    if (!rc) rc = xfer_d2h(ctx, xy_out, k.xy_out, (size_t)n * 8);
    if (!rc) rc = xfer_d2h(ctx, status_out, k.status, (size_t)n);
    if (!rc) rc = xfer_d2h(ctx, iters_out, k.iters, (size_t)n * 4);
    if (rc) { (void)xfer_flush(ctx); return rc; }
    return xfer_flush(ctx);
}

extern "C" int vo_klt_track(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int iters, double eps, double min_eig, double fb, float* xy_out,
                            uint8_t* status_out, int32_t* iters_out, int cap, int* n_out)
{
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !xy_out || !status_out || !n_out || cap < 0)
        return vo_fail(ctx, VO_E_ARG, "vo_klt_track: bad argument");
    KltPrm prm;
    if (int rc = klt_params(ctx, win, levels, iters, eps, min_eig, fb, "vo_klt_track", &prm)) return rc;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_pair || !b.has_pair) return vo_fail(ctx, VO_E_STATE, "vo_klt_track: slots %d and %d must both hold a pair", slot_a, slot_b);
    if (!a.has_kp || a.n_kp <= 0) return vo_fail(ctx, VO_E_STATE, "vo_klt_track: slot %d holds no keypoints", slot_a);
    if (a.w != b.w || a.h != b.h) return vo_fail(ctx, VO_E_STATE, "vo_klt_track: the slots' images differ in shape (%dx%d, %dx%d)", a.w, a.h, b.w, b.h);
    const int n = a.n_kp;
    if (n > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "vo_klt_track: %d keypoints exceed capacity %d", n, ctx->kp_cap);
    if (n > cap) return vo_fail(ctx, VO_E_CAP, "%d keypoints exceed the output capacity %d", n, cap);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = klt_ws_prepare(ctx)) return rc;
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    KltWs& k = ctx->mw->klt;
    if (ctx->has_roi) { prm.ox = (double)ctx->roi[0]; prm.oy = (double)ctx->roi[1]; }
    int rc = klt_enqueue(ctx, a.left, b.left, a.w, a.h, prm, fb > 0, a.kp_xy, n);
    if (!rc) rc = xfer_d2h(ctx, xy_out, k.xy_out, (size_t)n * 8);
    if (!rc) rc = xfer_d2h(ctx, status_out, k.status, (size_t)n);
    if (!rc && iters_out) rc = xfer_d2h(ctx, iters_out, k.iters, (size_t)n * 4);
    if (rc) { (void)xfer_flush(ctx); return rc; }
    if ((rc = xfer_flush(ctx))) return rc;
    *n_out = n;
    return VO_OK;
}

// =========================================================================================
// Lucas-Kanade PnP pair step (vo_klt_pnp_pair / _begin / _end): what StereoOdometer(match="klt", pose_method="pnp") composes out of
// vo_klt_track -> host filter -> vo_points3d_at -> vo_ransac_pnp, as ONE chain on ctx->stream -- the pyramid launches, the forward
// (and backward) tracking launch, k_klt_pnp_prep (geom.hip), then the tail of the stereo PnP step (pnp_tail_enqueue: k_pnp_hyp,
// k_pnp_score, k_pnp_finish).  No copy command, ONE host synchronisation; the record and the arrays are written into pinned
// memory by the kernels.  The halves run the chain on a POSE alternate, in that alternate's own Lucas-Kanade workspace.
// =========================================================================================
static int klt_pnp_check(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int klt_iters, double eps, double min_eig, double fb,
                         const double* K4v, int iters, float thr, int refine_iters, int lo_rounds, const char* who, KltPrm* prm)
{
    if (!ctx || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS || !K4v) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (int rc = klt_params(ctx, win, levels, klt_iters, eps, min_eig, fb, who, prm)) return rc;
    if (int rc = pnp_ranges_check(ctx, K4v, iters, thr, refine_iters, who)) return rc;
    if (int rc = pnp_lo_check(ctx, lo_rounds, refine_iters, who)) return rc;
    const FrameSlot& a = ctx->slots[slot_a];
    const FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_pair || !b.has_pair) return vo_fail(ctx, VO_E_STATE, "%s: slots %d and %d must both hold a pair", who, slot_a, slot_b);
    if (!a.has_kp) return vo_fail(ctx, VO_E_STATE, "%s: slot %d holds no keypoints", who, slot_a);
    if (a.w != b.w || a.h != b.h) return vo_fail(ctx, VO_E_STATE, "%s: the slots' images differ in shape (%dx%d, %dx%d)", who, a.w, a.h, b.w, b.h);
    if (!slot_sparse(a) && !a.has_disp) return vo_fail(ctx, VO_E_STATE, "%s: slot %d needs disparity (or keypoints that carry depth)", who, slot_a);
    if (!ctx->has_Q) return vo_fail(ctx, VO_E_STATE, "vo_set_Q has not been called");
    if (a.n_kp > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "%s: %d keypoints exceed capacity %d", who, a.n_kp, ctx->kp_cap);
    if (ctx->has_roi) { prm->ox = (double)ctx->roi[0]; prm->oy = (double)ctx->roi[1]; }
    return VO_OK;
}

// the whole chain on ctx->stream, in the match scratch in force; rec / arr: pinned host memory the kernels write (arr may be NULL:
// mask, q, t as the PnP step lays them out, then the tracked positions from byte 9 pnp_cap on)
static int klt_pnp_enqueue(vo_ctx* ctx, FrameSlot& a, FrameSlot& b, const KltPrm& prm, bool fb, const double* K4v, int iters, float thr, uint32_t seed,
                           int refine_iters, int lo_rounds, PnpRec* rec, uint8_t* arr)
{
    int rc;
    if ((rc = klt_ws_prepare(ctx))) return rc;
    PnpWs w;
    if ((rc = pnp_ws_take(ctx, a.n_kp, iters, &w))) return rc;
    KltWs& k = ctx->mw->klt;
    if ((rc = klt_enqueue(ctx, a.left, b.left, a.w, a.h, prm, fb, a.kp_xy, a.n_kp))) return rc;
    StageTimer t(ctx, VO_T_POSE);
    if ((rc = klt_pnp_prep_launch(ctx, a, k.xy_out, k.status, w.d, arr ? (float*)(arr + pnp_cap(ctx->kp_cap) * 9) : nullptr))) return rc;
    return pnp_tail_enqueue(ctx, w, a.n_kp, K4v, iters, thr, seed, refine_iters, lo_rounds, rec, arr, nullptr);
}

static int klt_pnp_unpack(vo_ctx* ctx, const PnpRec* r, const uint8_t* arr, int nq, int lo_rounds, int32_t* counts4, int32_t* flags, double* Rt12,
                          double* Rt12_refined, int32_t* refine2, int32_t* lo2, uint8_t* mask_out, int32_t* q_idx, float* xy_out, const char* who)
{
    if (arr && xy_out && r->n > 0) memcpy(xy_out, arr + pnp_cap(ctx->kp_cap) * 9, (size_t)r->n * 8);
    return pnp_unpack(ctx, r, arr, nq, counts4, flags, Rt12, Rt12_refined, refine2, mask_out, q_idx, nullptr, who, lo_rounds, lo2);
}

extern "C" int vo_klt_pnp_pair(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int klt_iters, double eps, double min_eig, double fb,
                               const double* K4v, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds, int32_t* counts4,
                               int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2, int32_t* lo2, uint8_t* mask_out,
                               int32_t* q_idx, float* xy_out, int cap)
{
    const char* who = "vo_klt_pnp_pair";
    if (ctx && (!counts4 || !flags || !Rt12 || !refine2)) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    KltPrm prm;
    int rc = klt_pnp_check(ctx, slot_a, slot_b, win, levels, klt_iters, eps, min_eig, fb, K4v, iters, thr, refine_iters, lo_rounds, who, &prm);
    if (rc) return rc;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    const bool want = mask_out || q_idx || xy_out;
    if (want && cap < a.n_kp) return vo_fail(ctx, VO_E_CAP, "%s: outputs hold %d entries, %d keypoints", who, cap, a.n_kp);
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    PnpRec* rec = (PnpRec*)ctx->pinned;
    pnp_rec_clear(rec);
    uint8_t* arr = nullptr;
    if (a.n_kp > 0) {
        const size_t bytes = pnp_cap(ctx->kp_cap) * PNP_ARR;
        if (want && !(arr = (uint8_t*)xfer_stage(ctx, bytes))) {
            if ((rc = xfer_flush(ctx))) return rc;
            if (!(arr = (uint8_t*)xfer_stage(ctx, bytes))) return vo_fail(ctx, VO_E_CAP, "%s: the transfer arena cannot hold %d keypoints", who, a.n_kp);
        }
        if ((rc = klt_pnp_enqueue(ctx, a, b, prm, fb > 0, K4v, iters, thr, seed, refine_iters, lo_rounds, rec, arr))) { (void)xfer_flush(ctx); return rc; }
        if ((rc = xfer_flush(ctx))) return rc;       // the one synchronisation
        if (!slot_sparse(a) && (rc = slot_health(ctx, a, slot_a))) return rc;       // never a pose from an undefined disparity (b's is not read)
    }
    return klt_pnp_unpack(ctx, rec, arr, a.n_kp, lo_rounds, counts4, flags, Rt12, Rt12_refined, refine2, lo2, mask_out, q_idx, xy_out, who);
}

extern "C" int vo_klt_pnp_pair_begin(vo_ctx* ctx, int slot_a, int slot_b, int win, int levels, int klt_iters, double eps, double min_eig, double fb,
                                     const double* K4v, int iters, float thr, uint32_t seed, int refine_iters, int lo_rounds, int want_arrays,
                                     int* ticket_out)
{
    const char* who = "vo_klt_pnp_pair_begin";
    if (ctx && !ticket_out) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    KltPrm prm;
    int rc = klt_pnp_check(ctx, slot_a, slot_b, win, levels, klt_iters, eps, min_eig, fb, K4v, iters, thr, refine_iters, lo_rounds, who, &prm);
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
        rc = klt_pnp_enqueue(ctx, a, b, prm, fb > 0, K4v, iters, thr, seed, refine_iters, lo_rounds, (PnpRec*)p.result,
                             want_arrays ? p.result + PNP_HDR : nullptr);
    }
    if (rc) return rc;
    p.slot_a = slot_a; p.slot_b = slot_b;
    p.gen_a = slot_sparse(a) ? 0 : a.disp_gen;       // (keypoints that carry depth: the step read no disparity, nothing to check at _end)
    p.gen_b = !slot_sparse(a) && b.has_disp ? b.disp_gen : 0;
    p.pnp = true; p.klt = true; p.want = want_arrays != 0 && a.n_kp > 0; p.nq = a.n_kp; p.lo = lo_rounds;
    return alt_close(ctx, vo_ctx::ALT_POSE, k, a, b, ticket_out);
}

extern "C" int vo_klt_pnp_pair_end(vo_ctx* ctx, int ticket, int32_t* counts4, int32_t* flags, double* Rt12, double* Rt12_refined, int32_t* refine2,
                                   int32_t* lo2, uint8_t* mask_out, int32_t* q_idx, float* xy_out, int cap)
{
    const char* who = "vo_klt_pnp_pair_end";
    int rc = alt_ticket(ctx, vo_ctx::ALT_POSE, ticket, counts4 && flags && Rt12 && refine2, who);
    if (rc) return rc;
    vo_ctx::PoseAlt& p = ctx->pose_alt[ticket];
    if (!p.klt)
        return vo_fail(ctx, VO_E_STATE, "%s: ticket %d belongs to %s (end it with %s)", who, ticket, p.pnp ? "vo_pnp_pair_begin" : "vo_pose_pair_begin",
                       p.pnp ? "vo_pnp_pair_end" : "vo_pose_pair_end");
    if ((mask_out || q_idx || xy_out) && p.nq > 0 && (!p.want || cap < p.nq))
        return vo_fail(ctx, VO_E_CAP, "%s: outputs hold %d entries, %d keypoints (or the step was begun without want_arrays)", who, cap, p.nq);
    if ((rc = alt_wait(ctx, p))) return rc;
    const int32_t gens[2] = { p.gen_a, p.gen_b };
    const int slots[2] = { p.slot_a, p.slot_b };
    for (int i = 0; i < 2; i++) {
        const FrameSlot& f = ctx->slots[slots[i]];
        if (gens[i] != 0 && *(volatile int32_t*)f.sweep_word == gens[i])
            return vo_fail(ctx, VO_E_SWEEP, "Lucas-Kanade PnP step %d: the aggregation sweep of the pair in slot %d gave up a strip hand-off: its "
                                            "disparity is undefined and no pose is derived from it", ticket, slots[i]);
    }
    return klt_pnp_unpack(ctx, (const PnpRec*)p.result, p.want ? p.result + PNP_HDR : nullptr, p.nq, p.lo, counts4, flags, Rt12, Rt12_refined, refine2,
                          lo2, mask_out, q_idx, xy_out, who);
}
