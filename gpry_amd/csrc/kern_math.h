// Kernel algebra shared by the covariance kernels (kernel_build.hip) and the resident predict kernel (server.hip):
// parameter blocks, correlation functions restated from sklearn:kernels.py:1553-1580 (RBF), :1708-1768 (Matern),
// :1239-1291 (Constant), and the per-slice posterior mean of one point.
#pragma once
#include "common.h"

struct KernParams {
    double C;
    int d, dpad, has_aff;
    int64_t N;
    double white;       // w of a model with GPRY_KERNEL_WHITE (on the diagonal of the training matrix: C + (noise + w))
    int white_on;       // 0: no white term -- the diagonal keeps the expression it had, C + noise
};
struct AffParams {
    double ls[GPRY_MAX_DIM];     // length scales (unused slots = 1)
    double lo[GPRY_MAX_DIM];
    double span[GPRY_MAX_DIM];
};

#define SQRT3 1.7320508075688772
#define SQRT5 2.23606797749979

template <int KID>
__device__ __forceinline__ double corr_r2(double r2) {
    if (KID == GPRY_RBF) return exp(-0.5 * r2);
    if (KID == GPRY_MATERN12) return exp(-sqrt(r2));
    if (KID == GPRY_MATERN32) { double t = sqrt(r2) * SQRT3; return (1.0 + t) * exp(-t); }
    double t = sqrt(r2) * SQRT5;
    return (1.0 + t + t * t * (1.0 / 3.0)) * exp(-t);
}
// Straight-line sqrt / exp for the cross-kernel panel (4.1e9 evaluations per 1e6 candidates at
// N = 4096: the panel build is VALU-bound, and libm's versions carry range checks, denormal
// scaling and ~10 register moves each).  Valid for the arguments that occur here: x >= 0 not
// denormal; t >= 0.  Accuracy ~1 ulp.
__device__ __forceinline__ double fast_sqrt_pos(double x) {
    const double s = __builtin_amdgcn_rsq(x);
    double g = x * s, h = 0.5 * s;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    double e = fma(-g, g, x);
    g = fma(e, h, g);
    e = fma(-g, g, x);
    g = fma(e, h, g);
    return x == 0.0 ? 0.0 : g;
}
__device__ __forceinline__ double fast_exp_neg(double t) {      // exp(-t)
    const double y = -t;
    const double n = __builtin_rint(y * 1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, y);
    r = fma(n, -1.90821492927058770002e-10, r);
    // exp(r), |r| <= ln2/2: Taylor to degree 13 (truncation 4e-18 relative)
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const double nn = fmax(n, -1100.0);      // exp(-t) underflows to 0 through ldexp
    return __builtin_ldexp(p, (int)nn);
}
template <int KID>
__device__ __forceinline__ double corr_r2_fast(double r2) {
    if (KID == GPRY_RBF) return fast_exp_neg(0.5 * r2);
    if (KID == GPRY_MATERN12) return fast_exp_neg(fast_sqrt_pos(r2));
    if (KID == GPRY_MATERN32) { double t = fast_sqrt_pos(r2) * SQRT3; return (1.0 + t) * fast_exp_neg(t); }
    double t = fast_sqrt_pos(r2) * SQRT5;
    return (1.0 + t + t * t * (1.0 / 3.0)) * fast_exp_neg(t);
}
// ---- the correlation from a PRE-SCALED squared distance u = s r^2 (round 5, the MFMA panel of the sweep: 4.1e9
// evaluations per 1e6 candidates at N = 4096, FP64-issue-bound).  s = corr_scale<KID>(): 1/2 (RBF: k = e^-u), 1 (Matern-1/2:
// k = e^-sqrt(u)), 3 and 5 (Matern-3/2, -5/2: t = sqrt(u)); the caller folds s into the norms it adds anyway, which saves
// the multiplication by sqrt(3) / sqrt(5) behind the root.  Against corr_r2_fast per evaluation of Matern-5/2 (vector
// instructions, profiles/r05_kern_math.md): root 12 -> 8 (no zero test: u >= 1e-290 is the caller's clamp, where k = 1 to
// the last bit; one correction step instead of two), polynomial 3 -> 2 (Horner), exponential 20 -> 18 (degree 11 instead
// of 13 on |r| <= ln 2 / 2: interpolant at the Chebyshev nodes, 1.5e-16 relative including the rounding of its Horner form
// -- the Taylor polynomial needs two more terms for that).  Root and exponential within 1 ulp of the correctly rounded
// values on 4e6 log-uniform arguments, like libm's and corr_r2_fast's (tools/r05/kern_math_check.hip); not the same bits.
template <int KID>
__host__ __device__ constexpr double corr_scale() {
    return KID == GPRY_RBF ? 0.5 : KID == GPRY_MATERN12 ? 1.0 : KID == GPRY_MATERN32 ? 3.0 : 5.0;
}
__device__ __forceinline__ double fast_sqrt_nz(double x) {         // x >= 1e-290, not denormal
    const double s = __builtin_amdgcn_rsq(x);
    double g = x * s, h = 0.5 * s;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    const double e = fma(-g, g, x);
    return fma(e, h, g);        // ONE correction behind the coupled step: <= 1 ulp over 4e6 arguments, as with two (kern_math_check)
}
__device__ __forceinline__ double fast_exp_neg11(double t) {       // exp(-t), t >= 0
    const double n = __builtin_rint(t * -1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, -t);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 2.5107785307679967e-08;
    p = fma(p, r, 2.7632571010826906e-07);
    p = fma(p, r, 2.7557247099675525e-06);
    p = fma(p, r, 2.480148569156966e-05);
    p = fma(p, r, 0.00019841269885093954);
    p = fma(p, r, 0.0013888888952097655);
    p = fma(p, r, 0.008333333333320085);
    p = fma(p, r, 0.04166666666648896);
    p = fma(p, r, 0.16666666666666685);
    p = fma(p, r, 0.5000000000000018);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)fmax(n, -1100.0));             // underflows to 0 through ldexp
}
template <int KID>
__device__ __forceinline__ double corr_scaled_fast(double u) {
    if (KID == GPRY_RBF) return fast_exp_neg11(u);
    const double t = fast_sqrt_nz(u);
    if (KID == GPRY_MATERN12) return fast_exp_neg11(t);
    if (KID == GPRY_MATERN32) return (1.0 + t) * fast_exp_neg11(t);
    return fma(fma(t, 1.0 / 3.0, 1.0), t, 1.0) * fast_exp_neg11(t);
}
// returns k(r) in *kval and h with d k / d log l_k = h * D_k   (both without the factor C)
template <int KID>
__device__ __forceinline__ double corr_and_h(double r2, double* kval) {
    if (KID == GPRY_RBF) { double e = fast_exp_neg(0.5 * r2); *kval = e; return e; }
    if (KID == GPRY_MATERN12) {
        double r = fast_sqrt_pos(r2); double e = fast_exp_neg(r); *kval = e;
        return r != 0.0 ? e / r : 0.0;
    }
    if (KID == GPRY_MATERN32) {
        double t = fast_sqrt_pos(r2) * SQRT3; double e = fast_exp_neg(t);
        *kval = (1.0 + t) * e;
        return 3.0 * e;
    }
    double t = fast_sqrt_pos(r2) * SQRT5; double e = fast_exp_neg(t);
    *kval = (1.0 + t + t * t * (1.0 / 3.0)) * e;
    return (5.0 / 3.0) * (t + 1.0) * e;
}

static KernParams make_kp(gpry_ctx* ctx) {
    KernParams kp;
    kp.C = exp(ctx->theta[0]);
    kp.d = ctx->d; kp.dpad = ctx->dpad;
    kp.has_aff = ctx->tf.has_x_affine; kp.N = ctx->N;
    kp.white = ctx_white(ctx); kp.white_on = ctx->white ? 1 : 0;
    return kp;
}
static AffParams make_ap(gpry_ctx* ctx, bool use_affine) {
    AffParams ap;
    for (int k = 0; k < GPRY_MAX_DIM; k++) {
        // sklearn divides by the length scale (x / l); we keep the division, not a reciprocal
        // multiply, so that scaled coordinates round identically.
        ap.ls[k] = k < ctx->d ? exp(ctx->theta[1 + k]) : 1.0;
        ap.lo[k] = (use_affine && k < ctx->d) ? ctx->tf.x_lo[k] : 0.0;
        ap.span[k] = (use_affine && k < ctx->d) ? ctx->tf.x_span[k] : 1.0;
    }
    return ap;
}

#define DISPATCH_KID(kid, CALL)                         \
    switch (kid) {                                      \
        case GPRY_RBF: { CALL(GPRY_RBF); break; }       \
        case GPRY_MATERN12: { CALL(GPRY_MATERN12); break; } \
        case GPRY_MATERN32: { CALL(GPRY_MATERN32); break; } \
        default: { CALL(GPRY_MATERN52); break; }        \
    }
// the samplers' instantiations: CALL(DP, KID) with DP the smallest of 4 / 8 / 16 / 32 that holds d
#define DISPATCH_DP_(d, CALL, KID)                                          \
    if ((d) <= 4) { CALL(4, KID); } else if ((d) <= 8) { CALL(8, KID); }    \
    else if ((d) <= 16) { CALL(16, KID); } else { CALL(32, KID); }
#define DISPATCH_DP_KID(d, kid, CALL)                                       \
    switch (kid) {                                                          \
        case GPRY_RBF: { DISPATCH_DP_(d, CALL, GPRY_RBF) break; }           \
        case GPRY_MATERN12: { DISPATCH_DP_(d, CALL, GPRY_MATERN12) break; } \
        case GPRY_MATERN32: { DISPATCH_DP_(d, CALL, GPRY_MATERN32) break; } \
        default: { DISPATCH_DP_(d, CALL, GPRY_MATERN52) break; }            \
    }

// ------------------------------------------------------------------------------------
// One slice of the posterior mean of ONE point: sum over the training rows [row_lo, row_lo + rows_per_split) of
// alpha_j C k(x, X_j) in transformed units, by one workgroup of 256 threads (result valid in thread 0).  `x`: the d
// raw coordinates of the point (any address space the caller can read: mapped host memory, LDS, global).  Shared by
// the one-launch kernel (predict_mean_small_kernel) and the resident one (server.hip): whichever of the two serves
// a call, the bits are the same.
#define MEAN_SLICE_CH 4096        // rows per LDS chunk of the one-launch kernel
// CH: rows per chunk (the size of r2s).  `base`: Xs / alpha_ hold the rows from `base` on (0: the arrays of the context
// in global memory; row_lo: a copy of this slice that the resident kernel keeps in LDS) -- the values and the order of
// every sum are the same either way.
template <int DP, int KID, int CH = MEAN_SLICE_CH>
__device__ __forceinline__ double mean_slice(const double* x, const double* __restrict__ Xs, const double* __restrict__ alpha_,
                                             int64_t row_lo, int64_t rows_per_split, const KernParams& kp, const AffParams& ap,
                                             double* r2s /*[CH]*/, double* red /*[256]*/, int64_t base = 0) {
    constexpr int P = DP / 2;             // lanes per training row: one 16-byte piece each
    const int t = threadIdx.x, sub = t % P, rloc = t / P;
    // this lane's two scaled coordinates of the point
    double x0 = 0.0, x1 = 0.0;
    {
        const int k0 = 2 * sub, k1 = 2 * sub + 1;
        if (k0 < kp.d) { double v = x[k0]; if (kp.has_aff) v = (v - ap.lo[k0]) / ap.span[k0]; x0 = v / ap.ls[k0]; }
        if (k1 < kp.d) { double v = x[k1]; if (kp.has_aff) v = (v - ap.lo[k1]) / ap.span[k1]; x1 = v / ap.ls[k1]; }
    }
    const bool piece_ok = 2 * sub < kp.dpad;
    double acc = 0.0;
    const int64_t row_hi = (row_lo + rows_per_split < kp.N) ? row_lo + rows_per_split : kp.N;
    for (int64_t c0 = row_lo; c0 < row_hi; c0 += CH) {
        const int nrow = (int)((row_hi - c0 < CH) ? row_hi - c0 : CH);
        // phase 1: squared distances, rows read as whole cache lines (P lanes per row); eight
        // passes are loaded back to back so that their memory latencies overlap
        constexpr int RP = 256 / P;       // rows per pass
        for (int r0 = 0; r0 < nrow; r0 += 8 * RP) {
            double2 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int row = r0 + u * RP + rloc;
                v[u] = make_double2(0.0, 0.0);
                if (row < nrow && piece_ok)
                    v[u] = *reinterpret_cast<const double2*>(Xs + (c0 - base + row) * kp.dpad + 2 * sub);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int row = r0 + u * RP + rloc;
                const double d0 = x0 - v[u].x, d1 = x1 - v[u].y;
                double part = piece_ok ? fma(d1, d1, d0 * d0) : 0.0;
#pragma unroll
                for (int o = 1; o < P; o <<= 1) part += __shfl_xor(part, o);
                if (sub == 0 && row < nrow) r2s[row] = part;
            }
        }
        __syncthreads();
        // phase 2: one row per lane, four independent chains
        for (int j0 = t; j0 < nrow; j0 += 1024) {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = j0 + 256 * q;
                v[q] = j < nrow ? alpha_[c0 - base + j] * (kp.C * corr_r2_fast<KID>(r2s[j])) : 0.0;
            }
            acc += (v[0] + v[1]) + (v[2] + v[3]);
        }
        __syncthreads();
    }
    // The binary tree over the 256 partial sums -- red[t] += red[t + s] for s = 128, 64, ..., 1 -- with ONE barrier: the
    // two cross-wave levels are read back by wave 0, the six levels inside it are cross-lane adds with the same pairs
    // (t, t + s), so the result is the tree's to the last bit (the eight barriers of the loop form were 0.8 us of a
    // request the resident kernel answers in ~3).
    red[t] = acc;
    __syncthreads();
    double out = 0.0;
    if (t < 64) {
        double v = (red[t] + red[t + 128]) + (red[t + 64] + red[t + 192]);
        v += __shfl_down(v, 32);
        v += __shfl_down(v, 16);
        v += __shfl_down(v, 8);
        v += __shfl_down(v, 4);
        v += __shfl_down(v, 2);
        v += __shfl_down(v, 1);
        out = v;
    }
    __syncthreads();          // `red` may be reused by the caller's next point
    return out;
}

// One slice of the posterior mean of UP TO R POINTS in one pass over the training rows: every row and every alpha is
// loaded once and used for each active point.  x: the points' raw coordinates, point p at x + p * GPRY_MAX_DIM; mask: bit
// p set = point p is active (the same value in every thread; a point that is masked out costs nothing and out[p] is
// not written).  For every active point the arithmetic is mean_slice's, operation for operation: the two scaled
// coordinates per lane, fma(d1, d1, d0 * d0) and the xor-shuffle sum over the P lanes, phase 2's groups
// (v0 + v1) + (v2 + v3) of the rows j0 + 256 q in ascending j0, the one-barrier tree -- so out[p] (valid in thread 0)
// has the bits of mean_slice of point p alone.  The rows of r^2 are kept in chunks of MEAN_MULTI_CH = 1024 per point
// instead of 4096: thread t adds the same groups in the same order for any chunk size that is a multiple of 1024 (the
// CH parameter of mean_slice, which server.hip uses).  r2s: R x MEAN_MULTI_CH doubles; the tree's 256 partial sums of
// point p go through the first 256 of its chunk, which phase 2 has finished with by then.
#define MEAN_MULTI_CH 1024
template <int DP, int KID, int R>
__device__ __forceinline__ void mean_slice_multi(const double* x, unsigned mask, const double* __restrict__ Xs,
                                                 const double* __restrict__ alpha_, int64_t row_lo, int64_t rows_per_split,
                                                 const KernParams& kp, const AffParams& ap, double* r2s /*[R][MEAN_MULTI_CH]*/,
                                                 double (&out)[R]) {
    constexpr int P = DP / 2, CH = MEAN_MULTI_CH;
    const int t = threadIdx.x, sub = t % P, rloc = t / P;
    double x0[R], x1[R], acc[R];
#pragma unroll
    for (int p = 0; p < R; p++) {
        x0[p] = 0.0; x1[p] = 0.0; acc[p] = 0.0;
        if (mask >> p & 1u) {
            const double* xp = x + p * GPRY_MAX_DIM;
            const int k0 = 2 * sub, k1 = 2 * sub + 1;
            if (k0 < kp.d) { double v = xp[k0]; if (kp.has_aff) v = (v - ap.lo[k0]) / ap.span[k0]; x0[p] = v / ap.ls[k0]; }
            if (k1 < kp.d) { double v = xp[k1]; if (kp.has_aff) v = (v - ap.lo[k1]) / ap.span[k1]; x1[p] = v / ap.ls[k1]; }
        }
    }
    const bool piece_ok = 2 * sub < kp.dpad;
    const int64_t row_hi = (row_lo + rows_per_split < kp.N) ? row_lo + rows_per_split : kp.N;
    for (int64_t c0 = row_lo; c0 < row_hi; c0 += CH) {
        const int nrow = (int)((row_hi - c0 < CH) ? row_hi - c0 : CH);
        // phase 1: eight passes of rows loaded back to back, each used for every active point
        constexpr int RP = 256 / P;
        for (int r0 = 0; r0 < nrow; r0 += 8 * RP) {
            double2 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int row = r0 + u * RP + rloc;
                v[u] = make_double2(0.0, 0.0);
                if (row < nrow && piece_ok)
                    v[u] = *reinterpret_cast<const double2*>(Xs + (c0 + row) * kp.dpad + 2 * sub);
            }
#pragma unroll
            for (int p = 0; p < R; p++) {
                if (!(mask >> p & 1u)) continue;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int row = r0 + u * RP + rloc;
                    const double d0 = x0[p] - v[u].x, d1 = x1[p] - v[u].y;
                    double part = piece_ok ? fma(d1, d1, d0 * d0) : 0.0;
#pragma unroll
                    for (int o = 1; o < P; o <<= 1) part += __shfl_xor(part, o);
                    if (sub == 0 && row < nrow) r2s[p * CH + row] = part;
                }
            }
        }
        __syncthreads();
        // phase 2: one row per lane, four independent chains per point (one trip: CH = 1024)
        for (int j0 = t; j0 < nrow; j0 += 1024) {
            double al[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = j0 + 256 * q;
                al[q] = alpha_[c0 + (j < nrow ? j : 0)];
            }
#pragma unroll
            for (int p = 0; p < R; p++) {
                if (!(mask >> p & 1u)) continue;
                double v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = j0 + 256 * q;
                    v[q] = j < nrow ? al[q] * (kp.C * corr_r2_fast<KID>(r2s[p * CH + j])) : 0.0;
                }
                acc[p] += (v[0] + v[1]) + (v[2] + v[3]);
            }
        }
        __syncthreads();
    }
    // mean_slice's tree, once per active point, with the two barriers shared
#pragma unroll
    for (int p = 0; p < R; p++)
        if (mask >> p & 1u) r2s[p * CH + t] = acc[p];
    __syncthreads();
#pragma unroll
    for (int p = 0; p < R; p++) {
        if (!(mask >> p & 1u)) continue;
        const double* red = r2s + p * CH;
        double o = 0.0;
        if (t < 64) {
            double v = (red[t] + red[t + 128]) + (red[t + 64] + red[t + 192]);
            v += __shfl_down(v, 32);
            v += __shfl_down(v, 16);
            v += __shfl_down(v, 8);
            v += __shfl_down(v, 4);
            v += __shfl_down(v, 2);
            v += __shfl_down(v, 1);
            o = v;
        }
        out[p] = o;
    }
    __syncthreads();
}


// ------------------------------------------------------------------------------------
// Gates of ONE point (gpry_set_gates), shared by the resident predict kernel (server.hip) and the nested sampler
// (nested.hip), so that a point gets the same verdict whichever of the two evaluates it.
struct GateParams {
    const double* sv; const double* coef; const double* trust;
    int64_t nsv; double gamma, intercept;
    int positive_finite, has_trust;
};
static GateParams make_gp(gpry_ctx* ctx) {
    GateParams g;
    g.sv = ctx->gate_sv; g.coef = ctx->gate_coef; g.trust = ctx->gate_trust;
    g.nsv = ctx->gate_nsv; g.gamma = ctx->gate_gamma; g.intercept = ctx->gate_intercept;
    g.positive_finite = ctx->gate_positive_finite; g.has_trust = ctx->gate_has_trust;
    return g;
}
// GPRY_MASK_* bits of one point (raw coordinates x in LDS): the trust box on the raw coordinates, the SVM decision
// function sum_r coef_r exp(-gamma |x_ - sv_r|^2) + intercept on the transformed ones -- the per-pair arithmetic of
// gates_kernel (kernel_build.hip), the support vectors dealt out over the 256 threads and their terms added by the
// fixed LDS tree.  Valid in every thread.
__device__ __forceinline__ unsigned point_gate_bits(const double* x, const GateParams& a, const KernParams& kp,
                                                    const AffParams& ap, double* red) {
    const int t = threadIdx.x;
    unsigned bits = 0;
    if (a.has_trust) {
        for (int k = 0; k < kp.d; k++) {
            const double v = x[k];
            if (!(v >= a.trust[2 * k] && v <= a.trust[2 * k + 1])) bits |= GPRY_MASK_OUTSIDE_TRUST;
        }
    }
    if (a.nsv > 0) {
        double part = 0.0;
        for (int64_t r = t; r < a.nsv; r += 256) {
            double r2 = 0.0;
            for (int k = 0; k < kp.d; k++) {
                double v = x[k];
                if (kp.has_aff) v = (v - ap.lo[k]) / ap.span[k];
                const double df = v - a.sv[r * kp.d + k];
                r2 = fma(df, df, r2);
            }
            part = fma(a.coef[r], fast_exp_neg(a.gamma * r2), part);
        }
        red[t] = part;
        __syncthreads();
        for (int s2 = 128; s2 >= 1; s2 >>= 1) {
            if (t < s2) red[t] += red[t + s2];
            __syncthreads();
        }
        const double dec = red[0] + a.intercept;
        __syncthreads();
        const bool finite = a.positive_finite ? dec > 0.0 : !(dec > 0.0);
        if (!finite) bits |= GPRY_MASK_CLASSIFIED_INF;
    }
    return bits;
}
