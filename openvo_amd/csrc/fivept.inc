// Five-point minimal solver for the essential matrix (D. Nister, PAMI 2004) as a per-lane device function, and the
// hypothesis kernels built on it (BASELINE config 5; SURVEY 7.7 names the 5-point solver as the real cv2 path's
// estimator).  Included by ransac.hip.  A hypothesis = 6 hash-sampled matches, 5 solve, the 6th picks among the <= 10 real
// solutions by Sampson error.  Two launches: k_ransac_hyp5 (one lane per hypothesis) reduces the five matches to the
// degree-10 polynomial det B(z); k_ransac_roots5 (32 lanes per hypothesis) finds its real roots -- which was 5/6 of the
// one-lane-per-hypothesis version's 0.26 ms: up to 55 bisections of 24..52 steps in sequence -- with one lane per
// bracketing interval, evaluates the candidates one per lane and picks.  Every value is computed by the same float64
// operations in the same order as the sequential restatement (oracle/src/fivept.c), only by different lanes
// (-ffp-contract=off):
//   null space of the 5x9 epipolar system by Gauss-Jordan with full pivoting  ->  E = xX + yY + zZ + W
//   det E = 0 and (E E^T - tr/2) E = 0: ten cubics, written straight into the column order
//       [x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1], Gauss-Jordan on the left half
//   B(z) [x y 1]^T = 0 from three row pairs, det B(z) of degree 10
//   real roots in z and 1/z by isolating between the roots of successive derivatives (fixed bisection counts)
//   (x, y) from the cross product of two rows of B(z)
//
// Storage.  The two eliminations pivot on run-time rows, which in per-lane arrays means scratch memory (3.4 KB per
// lane in the first version, 0.58 ms for 5000 hypotheses).  Here every run-time-indexed array lives in LDS, element-major
// (element e of lane l at double index e * 64 + l: all 64 lanes touch one 512-byte row, no bank conflicts): the 5x9
// system, then the 10x20 system in the same 100 KB (one wave per workgroup).  Everything else is indexed by
// compile-time constants after unrolling (the monomial tables are constexpr, the derivative coefficients are products
// of constants) and stays in registers.

#define FP_LDS_DOUBLES (200 * 64)       // per wave: the 10x20 system, one column of 64 lanes per element

// out (10 quadratics [x2 y2 z2 xy xz yz x y z 1]) += s * a (x y z 1) * b (x y z 1)
__device__ __forceinline__ void fp_mul11(const double* a, const double* b, double s, double* out)
{
    constexpr int T[4][4] = { { 0, 3, 4, 6 }, { 3, 1, 5, 7 }, { 4, 5, 2, 8 }, { 6, 7, 8, 9 } };
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[T[i][j]] += s * (a[i] * b[j]);
}
// out (20 cubics in the elimination order above) += s * a (10 quadratics) * b (x y z 1)
__device__ __forceinline__ void fp_mul21(const double* a, const double* b, double s, double* out)
{
    constexpr int T[10][4] = { { 0, 2, 4, 5 }, { 3, 1, 6, 7 }, { 10, 13, 16, 17 }, { 2, 3, 8, 9 }, { 4, 8, 10, 11 },
                               { 8, 6, 13, 14 }, { 5, 9, 11, 12 }, { 9, 7, 14, 15 }, { 11, 14, 17, 18 }, { 12, 15, 18, 19 } };
#pragma unroll
    for (int i = 0; i < 10; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[T[i][j]] += s * (a[i] * b[j]);
}
template <int DEG>
__device__ __forceinline__ double fp_eval(const double* c, double z)
{
    double v = c[DEG];
#pragma unroll
    for (int k = DEG - 1; k >= 0; k--) v = v * z + c[k];
    return v;
}
template <int DA, int DB>
__device__ __forceinline__ void fp_pmul(const double* a, const double* b, double* r)
{
#pragma unroll
    for (int k = 0; k <= DA + DB; k++) r[k] = 0.0;
#pragma unroll
    for (int i = 0; i <= DA; i++)
#pragma unroll
        for (int j = 0; j <= DB; j++) r[i + j] += a[i] * b[j];
}

// one level of the derivative chain, by the 16 lanes of a sub-group (sl = lane within it, m16sh = bit position of the
// sub-group's lane 0 inside a wave ballot): roots of the K-th derivative of c inside [-1, 1], given the nb roots of the
// (K+1)-th in brk (LDS); the new roots replace them.  Lane s brackets interval s (between break points s - 1 and s; -1 and 1
// at the ends) and bisects it when the signs differ -- the intervals are independent, so this is the sequential loop's
// arithmetic value for value; the roots land in interval order, at most DEG of them (the sequential loop's `nn < DEG`).
// d^K c / dz^K has coefficients c[i+K] (i+K)(i+K-1)...(i+1), multiplied in that order.
template <int K>
__device__ __forceinline__ int fp_root_level_par(const double* c, double* brk, int nb, int sl, int m16sh)
{
    constexpr int DEG = 10 - K, ITERS = K ? 24 : 52;
    double ck[DEG + 1];
#pragma unroll
    for (int i = 0; i <= DEG; i++) {
        double v = c[i + K];
#pragma unroll
        for (int m = K; m >= 1; m--) v = v * (double)(i + m);
        ck[i] = v;
    }
    const bool mine = sl <= nb;
    const double a = (sl == 0 || !mine) ? -1.0 : brk[sl - 1], b = (sl < nb && mine) ? brk[sl] : 1.0;
    const double fa = fp_eval<DEG>(ck, a), fb = fp_eval<DEG>(ck, b);
    const bool has = mine && ((fa < 0.0) != (fb < 0.0));
    double lo = a, hi = b;
    const bool neg = fa < 0.0;
    for (int it = 0; it < ITERS; it++) {
        const double mid = 0.5 * (lo + hi), fm = fp_eval<DEG>(ck, mid);
        if ((fm < 0.0) == neg) lo = mid; else hi = mid;
    }
    const unsigned m16 = (unsigned)(__ballot(has) >> m16sh) & 0xFFFFu;
    const int at = __popc(m16 & ((1u << sl) - 1u));
    __builtin_amdgcn_wave_barrier();                 // every lane has read its break points (LDS serves a wave's accesses in order)
    if (has && at < DEG) brk[at] = 0.5 * (lo + hi);
    __builtin_amdgcn_wave_barrier();
    return min(__popc(m16), DEG);
}

// real roots of a degree-10 polynomial inside [-1, 1], increasing, left in brk[0 .. return value)
__device__ __forceinline__ int fp_roots_unit_par(const double* c, double* brk, int sl, int m16sh)
{
    int nb = 0;
    nb = fp_root_level_par<9>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<8>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<7>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<6>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<5>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<4>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<3>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<2>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<1>(c, brk, nb, sl, m16sh);
    nb = fp_root_level_par<0>(c, brk, nb, sl, m16sh);
    return nb;
}

// what k_ransac_hyp5 hands to k_ransac_roots5 per hypothesis, element-major ([element][hypothesis]: lanes write neighbours):
// det B(z) scaled to max |coefficient| 1 (11), B (3 x 3 polynomials of degree 4: 45), the entries of E as polynomials in
// (x, y, z, 1) (36), the sixth match (4), a flag (1: the reductions did not hit a singular system): FP_REC_DOUBLES (ransac_ws.h)

// x1, x2: 5 normalised points each (interleaved) -> this hypothesis' record (rec[e * stride]); false when a reduction hits a
// singular system (the hypothesis then scores nothing).  lds: this lane's column of the wave's LDS block (element e at
// lds[e * 64]).
__device__ bool fp_reduce(const double* x1, const double* x2, double* rec, size_t stride, double* lds)
{
    // ---- null space of the 5x9 system (LDS, Q(r, c) = element r * 9 + c) -----------------------------------------
#define FPQ(r, c) lds[((r) * 9 + (c)) * 64]
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const double a = x1[2 * s], b = x1[2 * s + 1], c = x2[2 * s], d = x2[2 * s + 1];
        const double r[9] = { c * a, c * b, c, d * a, d * b, d, a, b, 1.0 };
#pragma unroll
        for (int k = 0; k < 9; k++) FPQ(s, k) = r[k];
    }
    unsigned long long perm = 0x876543210ull;        // nibble k = original column now at position k
#pragma unroll
    for (int i = 0; i < 5; i++) {
        int pr = i, pc = i;
        double best = -1.0;
        for (int r = i; r < 5; r++)
            for (int c = i; c < 9; c++) {
                const double v = fabs(FPQ(r, c));
                if (v > best) { best = v; pr = r; pc = c; }
            }
        if (!(best > 1e-300)) return false;
        for (int c = 0; c < 9; c++) { const double t = FPQ(i, c); FPQ(i, c) = FPQ(pr, c); FPQ(pr, c) = t; }
        for (int r = 0; r < 5; r++) { const double t = FPQ(r, i); FPQ(r, i) = FPQ(r, pc); FPQ(r, pc) = t; }
        {
            const unsigned long long ni = (perm >> (4 * i)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
            perm &= ~((15ull << (4 * i)) | (15ull << (4 * pc)));
            perm |= (np << (4 * i)) | (ni << (4 * pc));   // (i == pc: both fields get the same nibble back)
        }
        const double inv = 1.0 / FPQ(i, i);
        double rowi[9];
#pragma unroll
        for (int c = 0; c < 9; c++) { rowi[c] = FPQ(i, c) * inv; FPQ(i, c) = rowi[c]; }
#pragma unroll
        for (int r = 0; r < 5; r++)
            if (r != i) {
                const double f = FPQ(r, i);
#pragma unroll
                for (int c = 0; c < 9; c++) FPQ(r, c) -= f * rowi[c];
            }
    }
    // entry k of E as a polynomial (coefficients of x, y, z, 1): through LDS (run-time rows), then registers
#define FPE(k, j) lds[(45 + (k) * 4 + (j)) * 64]
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int k = 0; k < 9; k++) FPE(k, j) = 0.0;
        FPE((int)((perm >> (4 * (5 + j))) & 15ull), j) = 1.0;
#pragma unroll
        for (int i = 0; i < 5; i++) FPE((int)((perm >> (4 * i)) & 15ull), j) = -FPQ(i, 5 + j);
    }
    double Ep[9][4];
#pragma unroll
    for (int k = 0; k < 9; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) Ep[k][j] = FPE(k, j);
#undef FPQ
#undef FPE
    // ---- the ten cubic constraints, one row at a time in registers, then into LDS: M(r, c) = element r * 20 + c ----
#define FPM(r, c) lds[((r) * 20 + (c)) * 64]
    {
        double row[20];
#pragma unroll
        for (int c = 0; c < 20; c++) row[c] = 0.0;
        double m01[10], m02[10], m12[10];
#pragma unroll
        for (int k = 0; k < 10; k++) m01[k] = m02[k] = m12[k] = 0.0;
        fp_mul11(Ep[4], Ep[8], 1.0, m12); fp_mul11(Ep[5], Ep[7], -1.0, m12);
        fp_mul11(Ep[3], Ep[8], 1.0, m02); fp_mul11(Ep[5], Ep[6], -1.0, m02);
        fp_mul11(Ep[3], Ep[7], 1.0, m01); fp_mul11(Ep[4], Ep[6], -1.0, m01);
        fp_mul21(m12, Ep[0], 1.0, row);
        fp_mul21(m02, Ep[1], -1.0, row);
        fp_mul21(m01, Ep[2], 1.0, row);
#pragma unroll
        for (int c = 0; c < 20; c++) FPM(0, c) = row[c];
    }
    {
        double G[3][3][10];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < 10; k++) G[i][j][k] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) {
#pragma unroll
                for (int k = 0; k < 3; k++) fp_mul11(Ep[i * 3 + k], Ep[j * 3 + k], 1.0, G[i][j]);
                if (j != i) {
#pragma unroll
                    for (int k = 0; k < 10; k++) G[j][i][k] = G[i][j][k];
                }
            }
        double tr[10];
#pragma unroll
        for (int k = 0; k < 10; k++) tr[k] = 0.5 * ((G[0][0][k] + G[1][1][k]) + G[2][2][k]);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 10; k++) G[i][i][k] -= tr[k];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double row[20];
#pragma unroll
                for (int c = 0; c < 20; c++) row[c] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; k++) fp_mul21(G[i][k], Ep[k * 3 + j], 1.0, row);
#pragma unroll
                for (int c = 0; c < 20; c++) FPM(1 + i * 3 + j, c) = row[c];
            }
    }
    // ---- Gauss-Jordan on the first ten columns (run-time pivot rows: LDS; the pivot column is a compile-time index) ----
#pragma unroll
    for (int c = 0; c < 10; c++) {
        int pr = c;
        double best = fabs(FPM(c, c));
        for (int r = c + 1; r < 10; r++) {
            const double v = fabs(FPM(r, c));
            if (v > best) { best = v; pr = r; }
        }
        if (!(best > 1e-300)) return false;
        double rowc[20];                             // the pivot row, in registers for the whole elimination step
#pragma unroll
        for (int k = 0; k < 20; k++) rowc[k] = FPM(pr, k);
        if (pr != c) {
#pragma unroll
            for (int k = 0; k < 20; k++) FPM(pr, k) = FPM(c, k);
        }
        const double inv = 1.0 / rowc[c];
#pragma unroll
        for (int k = 0; k < 20; k++) { rowc[k] *= inv; FPM(c, k) = rowc[k]; }
        for (int r = 0; r < 10; r++)
            if (r != c) {
                const double f = FPM(r, c);
                if (f != 0.0) {
#pragma unroll
                    for (int k = 0; k < 20; k++) FPM(r, k) -= f * rowc[k];
                }
            }
    }
    // ---- B(z): rows from (e,f) = (4,5), (6,7), (8,9); remaining columns 10..19 = [xz^2 xz x | yz^2 yz y | z^3 z^2 z 1] --
    double B[3][3][5];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double e[10], f[10];
#pragma unroll
        for (int k = 0; k < 10; k++) { e[k] = FPM(4 + 2 * r, 10 + k); f[k] = FPM(5 + 2 * r, 10 + k); }
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int o = 3 * v;
            B[r][v][0] = e[o + 2];
            B[r][v][1] = e[o + 1] - f[o + 2];
            B[r][v][2] = e[o] - f[o + 1];
            B[r][v][3] = -f[o];
            B[r][v][4] = 0.0;
        }
        B[r][2][0] = e[9];
        B[r][2][1] = e[8] - f[9];
        B[r][2][2] = e[7] - f[8];
        B[r][2][3] = e[6] - f[7];
        B[r][2][4] = -f[6];
    }
#undef FPM
    double det[11];
#pragma unroll
    for (int k = 0; k <= 10; k++) det[k] = 0.0;
    {
        double p[8], q[8], m[8], t6[7], t7[7], t10[11], m6[7];
        fp_pmul<3, 4>(B[1][1], B[2][2], p); fp_pmul<4, 3>(B[1][2], B[2][1], q);
#pragma unroll
        for (int k = 0; k <= 7; k++) m[k] = p[k] - q[k];
        fp_pmul<3, 7>(B[0][0], m, t10);
#pragma unroll
        for (int k = 0; k <= 10; k++) det[k] += t10[k];
        fp_pmul<3, 4>(B[1][0], B[2][2], p); fp_pmul<4, 3>(B[1][2], B[2][0], q);
#pragma unroll
        for (int k = 0; k <= 7; k++) m[k] = p[k] - q[k];
        fp_pmul<3, 7>(B[0][1], m, t10);
#pragma unroll
        for (int k = 0; k <= 10; k++) det[k] -= t10[k];
        fp_pmul<3, 3>(B[1][0], B[2][1], t6); fp_pmul<3, 3>(B[1][1], B[2][0], t7);
#pragma unroll
        for (int k = 0; k <= 6; k++) m6[k] = t6[k] - t7[k];
        fp_pmul<4, 6>(B[0][2], m6, t10);
#pragma unroll
        for (int k = 0; k <= 10; k++) det[k] += t10[k];
    }
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k <= 10; k++) if (fabs(det[k]) > mx) mx = fabs(det[k]);
    if (!(mx > 0.0)) return false;
#pragma unroll
    for (int k = 0; k <= 10; k++) rec[(size_t)k * stride] = det[k] / mx;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 5; k++) rec[(size_t)(11 + (r * 3 + c) * 5 + k) * stride] = B[r][c][k];
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) rec[(size_t)(56 + i * 4 + j) * stride] = Ep[i][j];
    return true;
}

// one candidate z: (x, y) from the cross product of two rows of B(z), E = xX + yY + zZ + W scaled to unit Frobenius norm,
// Sampson error of the sixth match; false when the candidate is degenerate
__device__ __forceinline__ bool fp_candidate(const double (*B)[3][5], const double (*Ep)[4], double z, double u1, double v1, double u2, double v2,
                                             double* F, double& d)
{
    double b[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) b[r][c] = fp_eval<4>(B[r][c], z);
    double bc0 = 0.0, bc1 = 0.0, bc2 = 0.0;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const int q = (p + 1) % 3;
        const double c0 = b[p][1] * b[q][2] - b[p][2] * b[q][1];
        const double c1 = b[p][2] * b[q][0] - b[p][0] * b[q][2];
        const double c2 = b[p][0] * b[q][1] - b[p][1] * b[q][0];
        if (fabs(c2) > fabs(bc2)) { bc0 = c0; bc1 = c1; bc2 = c2; }
    }
    if (!(fabs(bc2) > 1e-300)) return false;
    const double x = bc0 / bc2, y = bc1 / bc2;
    double nn = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F[i] = ((x * Ep[i][0] + y * Ep[i][1]) + z * Ep[i][2]) + Ep[i][3];
        nn += F[i] * F[i];
    }
    if (!(nn > 0.0) || nn != nn) return false;
    const double inv = 1.0 / sqrt(nn);
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = F[i] * inv;
    const double fx0 = (F[0] * u1 + F[1] * v1) + F[2], fx1 = (F[3] * u1 + F[4] * v1) + F[5], fx2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double ft0 = (F[0] * u2 + F[3] * v2) + F[6], ft1 = (F[1] * u2 + F[4] * v2) + F[7];
    const double num = (u2 * fx0 + v2 * fx1) + fx2;
    const double den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1;
    d = (num * num) / den;
    return true;
}

// one wave per workgroup: its 100 KB LDS block holds one column of 64 lanes per matrix element
__global__ void __launch_bounds__(64) k_ransac_hyp5(const float* __restrict__ p1, const float* __restrict__ p2, int n, K4 K,
                                                    int iters, uint32_t seed, double* __restrict__ rec, const int* __restrict__ n_dev)
{
    extern __shared__ double s_fp[];
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= iters) return;
    if (n_dev) n = *n_dev;
    double* const my = rec + h;
    const size_t stride = (size_t)iters;
    if (n < 6) { my[96 * stride] = 0.0; return; }
    int idx[6];
    rs_sample_distinct<6>(seed, h, n, idx);
    double a[12], b[12];
    for (int s = 0; s < 6; s++) {
        const int i = idx[s];
        a[2 * s] = ((double)p1[2 * i] - K.cx) / K.fx; a[2 * s + 1] = ((double)p1[2 * i + 1] - K.cy) / K.fy;
        b[2 * s] = ((double)p2[2 * i] - K.cx) / K.fx; b[2 * s + 1] = ((double)p2[2 * i + 1] - K.cy) / K.fy;
    }
    const bool ok = fp_reduce(a, b, my, stride, s_fp + (threadIdx.x & 63));
    my[92 * stride] = a[10]; my[93 * stride] = a[11]; my[94 * stride] = b[10]; my[95 * stride] = b[11];
    my[96 * stride] = ok ? 1.0 : 0.0;
}

// 32 lanes per hypothesis: lanes 0..15 find the roots of det B(z) in [-1, 1], lanes 16..31 those of the reversed polynomial
// (the roots with |z| > 1 as 1 / z); then one lane per candidate -- det's roots first, then the reciprocals, ten at most,
// exactly the order of the sequential loop -- evaluates E and the sixth match's Sampson error, and the smallest error wins
// (the first of equals: the sequential loop replaces its best only on a strictly smaller error).
__global__ void __launch_bounds__(256) k_ransac_roots5(const double* __restrict__ rec, K4 K, int iters, double* __restrict__ E_out,
                                                       float* __restrict__ F_out)
{
    __shared__ double s_brk[4][4][12];               // [wave][sub-group][break points / roots]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int grp = lane >> 5, gl = lane & 31, sg = gl >> 4, sl = gl & 15;
    const int h = (blockIdx.x * 4 + wv) * 2 + grp;
    const bool live = h < iters;
    const size_t stride = (size_t)iters;
    const double* const my = rec + (live ? h : 0);
    const bool ok = live && my[96 * stride] != 0.0;
    double c[11];
#pragma unroll
    for (int k = 0; k <= 10; k++) c[k] = ok ? my[(size_t)(sg ? 10 - k : k) * stride] : (k == 0 ? 1.0 : 0.0);
    double* const brk = s_brk[wv][grp * 2 + sg];
    const int nroots = fp_roots_unit_par(c, brk, sl, (grp * 2 + sg) * 16);
    // candidates: position of this lane's root in the sequential loop's list
    const double rt = sl < nroots ? brk[sl] : 0.0;
    const bool usable = sl < nroots && (sg == 0 || (fabs(rt) > 1e-12 && fabs(rt) < 1.0));
    const unsigned long long bal = __ballot(usable);
    const unsigned m_det = (unsigned)(bal >> (grp * 32)) & 0xFFFFu, m_rev = (unsigned)(bal >> (grp * 32 + 16)) & 0xFFFFu;
    const int pos = sg == 0 ? sl : __popc(m_det) + __popc(m_rev & ((1u << sl) - 1u));      // (det's roots are all usable: m_det = its first n0 bits)
    double F[9], d = 0.0;
    bool have = ok && usable && pos < 10;
    if (have) {
        double B[3][3][5], Ep[9][4];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++)
#pragma unroll
                for (int k = 0; k < 5; k++) B[r][cc][k] = my[(size_t)(11 + (r * 3 + cc) * 5 + k) * stride];
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) Ep[i][j] = my[(size_t)(56 + i * 4 + j) * stride];
        const double z = sg == 0 ? rt : 1.0 / rt;
        have = fp_candidate(B, Ep, z, my[92 * stride], my[93 * stride], my[94 * stride], my[95 * stride], F, d);
        have = have && d < 1e300;                    // (NaN compares false: never the best, as in `d < bestd`)
    }
    // smallest (d, pos) over the 32 lanes of the hypothesis
    double bd = have ? d : 1e300;
    int bp = have ? pos : 64, bl = gl;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int op = __shfl_xor(bp, o, 64), ol = __shfl_xor(bl, o, 64);
        if (od < bd || (od == bd && op < bp)) { bd = od; bp = op; bl = ol; }
    }
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double w = __shfl(F[k], grp * 32 + bl, 64);
        E[k] = bp < 64 ? w : 0.0;
    }
    if (live && gl == 0) rs_emit(E, K, h, E_out, F_out);
}
