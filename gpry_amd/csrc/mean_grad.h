// The x-gradient of the posterior mean of ONE point inside a sampler kernel: what gpry_predict_grad's mean_grad is
// (kernel_build.hip: gradx_kernel + gradx_contract_kernel; gpry/gpr.py:1236-1266 with gpry/kernels.py:257-278 RBF,
// :326-432 Matern), by one workgroup of 256 threads, beside mean_slice of kern_math.h and with its flop shape: one pass
// over the training rows, N (3 d + 27) flops.  Used by hmc_chain_kernel (hmc.hip).
//
// With diff = x / l - X_j / l (the kernel's coordinates, Xs holds the scaled rows), r = |diff| and
//   w(r) = -exp(-r^2/2) (RBF),  -exp(-r)/r (Matern 1/2; r = 0: the reference's fill value, diff/l -> 1/l),
//          -3 exp(-sqrt3 r) (Matern 3/2),  -(5/3) (1 + sqrt5 r) exp(-sqrt5 r) (Matern 5/2),
// the gradient in the kernel's coordinates is  C / l_k  sum_j alpha_j w(r_j) diff_jk.
//
// Every thread strides the rows t, t + 256, ... of each slice and keeps DP partial sums in registers (DP = 32: 32 FP64
// accumulators, 64 VGPRs; all indices are compile-time, nothing goes to scratch).  The sums are then reduced in a fixed
// order: inside a wave by cross-lane moves (offsets 32, 16, ..., 1), across the four waves through LDS as
// (w0 + w1) + (w2 + w3).  The bits depend on the model and the point alone.
#pragma once
#include "kern_math.h"

#define MEAN_GRAD_LDS (4 * GPRY_MAX_DIM)        // doubles of LDS the reduction uses

// `xs`: the point's DP scaled coordinates in LDS (x / l after the model's affine map; slots >= d hold 0).  Adds this
// thread's rows of [row_lo, row_hi) to acc.
template <int DP, int KID>
__device__ __forceinline__ void mean_grad_rows(const double* xs, const double* __restrict__ Xs, const double* __restrict__ alpha_,
                                               int64_t row_lo, int64_t row_hi, const KernParams& kp, double (&acc)[DP]) {
    constexpr int P = DP / 2;
    double xr[DP];
#pragma unroll
    for (int k = 0; k < DP; k++) xr[k] = xs[k];
    for (int64_t j = row_lo + threadIdx.x; j < row_hi; j += 256) {
        double diff[DP];
        double r2 = 0.0;
#pragma unroll
        for (int p = 0; p < P; p++) {
            double2 v = make_double2(0.0, 0.0);
            if (2 * p < kp.dpad) v = *reinterpret_cast<const double2*>(Xs + j * kp.dpad + 2 * p);
            diff[2 * p] = 2 * p < kp.d ? xr[2 * p] - v.x : 0.0;
            diff[2 * p + 1] = 2 * p + 1 < kp.d ? xr[2 * p + 1] - v.y : 0.0;
            r2 = fma(diff[2 * p], diff[2 * p], r2);
            r2 = fma(diff[2 * p + 1], diff[2 * p + 1], r2);
        }
        double w;
        if (KID == GPRY_RBF) w = -fast_exp_neg(0.5 * r2);
        else if (KID == GPRY_MATERN12) { const double r = fast_sqrt_pos(r2); w = r != 0.0 ? -fast_exp_neg(r) / r : -1.0; }
        else if (KID == GPRY_MATERN32) w = -3.0 * fast_exp_neg(fast_sqrt_pos(r2) * SQRT3);
        else { const double tt = fast_sqrt_pos(r2) * SQRT5; w = -(5.0 / 3.0) * (1.0 + tt) * fast_exp_neg(tt); }
        w *= alpha_[j];
        if (KID == GPRY_MATERN12 && r2 == 0.0) {
#pragma unroll
            for (int k = 0; k < DP; k++) acc[k] += k < kp.d ? w : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < DP; k++) acc[k] = fma(w, diff[k], acc[k]);
        }
    }
}

// The gradient of the transformed mean at the point whose scaled coordinates are xs[0..DP) (LDS), over the slices of
// the one-point path (nsplit x rows_per_split, as ns_eval walks them): g[k] = C / l_k sum_j ..., k < d, written to LDS by
// threads k < d.  `lds`: MEAN_GRAD_LDS doubles.  Every thread of the workgroup calls it; g is valid after it returns.
template <int DP, int KID>
__device__ __forceinline__ void mean_grad(const double* xs, const double* __restrict__ Xs, const double* __restrict__ alpha_,
                                          int nsplit, int64_t rows_per_split, const KernParams& kp, const AffParams& ap,
                                          double* lds, double* g) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc[DP];
#pragma unroll
    for (int k = 0; k < DP; k++) acc[k] = 0.0;
    for (int s = 0; s < nsplit; s++) {
        const int64_t row_lo = (int64_t)s * rows_per_split;
        const int64_t row_hi = row_lo + rows_per_split < kp.N ? row_lo + rows_per_split : kp.N;
        mean_grad_rows<DP, KID>(xs, Xs, alpha_, row_lo, row_hi, kp, acc);
    }
#pragma unroll
    for (int k = 0; k < DP; k++) {
        double v = acc[k];
        v += __shfl_down(v, 32);
        v += __shfl_down(v, 16);
        v += __shfl_down(v, 8);
        v += __shfl_down(v, 4);
        v += __shfl_down(v, 2);
        v += __shfl_down(v, 1);
        if (lane == 0) lds[wave * GPRY_MAX_DIM + k] = v;
    }
    __syncthreads();
    if (t < kp.d) {
        const double v = (lds[t] + lds[GPRY_MAX_DIM + t]) + (lds[2 * GPRY_MAX_DIM + t] + lds[3 * GPRY_MAX_DIM + t]);
        g[t] = kp.C * v / ap.ls[t];
    }
    __syncthreads();
}
