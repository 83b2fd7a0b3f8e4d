// The N x N solve and the twist update of a Gauss-Newton step, shared by the PnP refit (ransac.hip: pn_gn_step) and the direct
// alignment (direct.hip: k_direct_align with 6 unknowns, k_direct_align_ab with 6 and 8): all compile this text.
#pragma once
#include <math.h>

// One Gauss-Newton step's solve in one lane: H (N x N, symmetric, upper triangle in packed row order) d = -g by Cholesky, every index
// a compile-time constant so that the factor stays in registers.  false: a pivot was not positive.  The operations of an unknown
// depend on N only through the loop bounds, so N = 6 is the sequence of operations pn_solve6 has always been.
template <int N>
__device__ __forceinline__ bool pn_solve(const double* Hp, const double* g, double* d)
{
    double L[N][N];
#pragma unroll
    for (int i = 0, k = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++, k++) L[j][i] = Hp[k];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        ok = ok && s > 0.0;
        const double dj = sqrt(s);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / dj;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    return ok;
}

__device__ __forceinline__ bool pn_solve6(const double* Hp, const double* g, double* d) { return pn_solve<6>(Hp, g, d); }

// Rt <- [Exp(w) R | Exp(w) t + v]   (Rodrigues; the series below 1e-4 rad, where sin / cos lose digits in the quotients)
__device__ __forceinline__ void pn_apply_twist(double* Rt, const double* d)
{
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
    double A, B;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double W[9] = { 0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0 };
    const double w3[3] = { wx, wy, wz };
    double E[9], out[12];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) E[r * 3 + c] = ((r == c ? 1.0 : 0.0) + A * W[r * 3 + c]) + B * (w3[r] * w3[c] - (r == c ? th2 : 0.0));
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) out[r * 4 + c] = (E[r * 3] * Rt[c] + E[r * 3 + 1] * Rt[4 + c]) + E[r * 3 + 2] * Rt[8 + c];
    for (int r = 0; r < 3; r++) out[r * 4 + 3] += d[3 + r];
    for (int k = 0; k < 12; k++) Rt[k] = out[k];
}
