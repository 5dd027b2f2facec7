// One entry of a Kriging-believer Gram row, shared by kb_gram_kernel (api.hip: one row per launch) and kb_gram_rows_kernel
// (kb_rank.hip: several rows per launch), so that a row has the same bits whatever shares its launch.
#pragma once
#include "common.h"

__device__ __forceinline__ double kb_corr(int kid, double r2) {
    switch (kid) {
        case GPRY_RBF: return exp(-0.5 * r2);
        case GPRY_MATERN12: return exp(-sqrt(r2));
        case GPRY_MATERN32: { double t = sqrt(r2) * 1.7320508075688772; return (1.0 + t) * exp(-t); }
        default: { double t = sqrt(r2) * 2.23606797749979; return (1.0 + t + t * t / 3.0) * exp(-t); }
    }
}
// one wave per (x, p): out_dot[x] = U[x].U[p] (stride-64 fma per lane, xor butterfly); out_k[x] = C k(|xs_x - xs_p|)
__device__ __forceinline__ void kb_gram_entry(const double* __restrict__ U, int64_t ldu, int64_t x, int64_t p, int64_t Np,
                                              const double* __restrict__ Xkb, int dpad, int kid, double C,
                                              double* __restrict__ out_dot, double* __restrict__ out_k) {
    const int lane = threadIdx.x & 63;
    const double* ux = U + x * ldu; const double* up = U + p * ldu;
    double s = 0.0;
    for (int64_t i = lane; i < Np; i += 64) s = fma(ux[i], up[i], s);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        out_dot[x] = s;
        double r2 = 0.0;
        for (int k = 0; k < dpad; k++) { double df = Xkb[x * dpad + k] - Xkb[p * dpad + k]; r2 = fma(df, df, r2); }
        out_k[x] = C * kb_corr(kid, r2);
    }
}
