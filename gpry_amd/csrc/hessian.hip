// Value, gradient and Hessian of the surrogate's posterior mean at a batch of points: the kernel behind
// gpry_hessian_mean.  What is done with the matrices (the Gaussian approximation at a maximum, the Laplace evidence, a
// first inverse-Hessian guess for the ascents and a proposal for the chain samplers) is host-side, in
// gpry_amd/maximize.py: hessian_gp, laplace_gp, covmat="laplace".
//
// The reference stops at first derivatives (gpry/gpr.py:1236-1266 with gpry/kernels.py:257-278 RBF, :326-432 Matern);
// the second ones follow from the same closed forms.  With diff_j = x / l - X_j / l (the kernel's coordinates, Xs holds
// the scaled rows), r = |diff_j|, w(r) as in mean_grad.h and q(r) = w'(r) / r:
//   q = exp(-r^2/2) (RBF),  3 sqrt3 exp(-sqrt3 r) / r (Matern 3/2; 0 at r = 0, the limit of q diff diff^T),
//       (25/3) exp(-sqrt5 r) (Matern 5/2),
//   S_ab = sum_j alpha_j q_j diff_ja diff_jb,   T = sum_j alpha_j w_j,   G_a = sum_j alpha_j w_j diff_ja,
//   g_a = y_std C G_a / (l_a span_a),   H_ab = y_std C (S_ab + T delta_ab) / (l_a l_b span_a span_b)
// in raw coordinates and units of y (span = 1 without the x-affine map): of the unclipped, ungated mean.  Matern 1/2 is
// refused: its mean has a kink at every training row.
//
// One 256-thread workgroup per point.  y is ns_eval of the point (gpr.predict(x[None]) bit for bit).  S is the weighted
// Gram D^T diag(alpha q) D, formed with v_mfma_f64_16x16x4: a wave walks its rows four at a time, lane (g = lane >> 4,
// r = lane & 15) holds coordinate r (and 16 + r for d > 16) of row g of the four; the A operand is (alpha_j q_j) diff,
// the B operand diff (operand and accumulator layout: chol16.h), r^2 of a row is summed over its 16 lanes.  d <= 16: one
// 16 x 16 accumulator tile; d > 16: the three lower tiles (low-low, high-low, high-high), mirrored on the way out.  T and
// G ride in the same pass.  The slices of the one-point path are walked in slice order, the four waves are combined
// through LDS as (w0 + w1) + (w2 + w3): the bits depend on the model and the point alone.  Only the lower triangle is
// computed; the upper one is its copy, so H is symmetric to the last bit.
#include "ns_common.h"

#define HESS_WSTRIDE 816          // doubles of LDS per wave: 3 tiles x 256, G (32), T (1), padded
#define HESS_G_OFF 768
#define HESS_T_OFF 800

// alpha_j q(r) and alpha_j w(r) of one row from its r^2
template <int KID>
__device__ __forceinline__ void hess_weights(double r2, double al, double* cq, double* cw) {
    if (KID == GPRY_RBF) {
        const double e = fast_exp_neg(0.5 * r2);
        *cq = al * e; *cw = -(al * e);
    } else if (KID == GPRY_MATERN32) {
        const bool z = !(r2 >= 1e-280);                       // r = 0 (and below fast_sqrt_pos's range): q diff diff^T -> 0
        const double r = fast_sqrt_pos(z ? 1.0 : r2);
        const double e = fast_exp_neg(r * SQRT3);
        *cq = z ? 0.0 : al * ((3.0 * SQRT3) * e / r);
        *cw = z ? -3.0 * al : -3.0 * (al * e);
    } else {
        const double tt = fast_sqrt_pos(r2) * SQRT5;
        const double e = fast_exp_neg(tt);
        *cq = al * ((25.0 / 3.0) * e);
        *cw = -(5.0 / 3.0) * (al * ((1.0 + tt) * e));
    }
}

template <int DP, int KID>
__global__ __launch_bounds__(256) void hessian_kernel(NsArgs a, KernParams kp, AffParams ap, const double* __restrict__ X,
                                                      double* __restrict__ y_out, double* __restrict__ g_out,
                                                      double* __restrict__ H_out) {
    constexpr bool WIDE = DP > 16;
    __shared__ double r2s[MEAN_SLICE_CH];        // ns_eval's rows of r^2, then the waves' partial sums
    __shared__ double red[256];
    __shared__ double s_x[GPRY_MAX_DIM];
    __shared__ double s_y;
    static_assert(4 * HESS_WSTRIDE <= MEAN_SLICE_CH, "the waves' partial sums reuse r2s");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4, d = kp.d;
    const int64_t p = blockIdx.x;
    if (t < GPRY_MAX_DIM) s_x[t] = t < d ? X[p * d + t] : 0.0;
    __syncthreads();
    const double y = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);

    // this lane's scaled coordinates of the point (mean_slice's arithmetic)
    const bool ok0 = r < d, ok1 = WIDE && 16 + r < d;
    double x0 = 0.0, x1 = 0.0;
    if (ok0) { double v = s_x[r]; if (kp.has_aff) v = (v - ap.lo[r]) / ap.span[r]; x0 = v / ap.ls[r]; }
    if (ok1) { double v = s_x[16 + r]; if (kp.has_aff) v = (v - ap.lo[16 + r]) / ap.span[16 + r]; x1 = v / ap.ls[16 + r]; }

    v4d LL = {0.0, 0.0, 0.0, 0.0}, HL = {0.0, 0.0, 0.0, 0.0}, HH = {0.0, 0.0, 0.0, 0.0};
    double G0 = 0.0, G1 = 0.0, T = 0.0;
    for (int s = 0; s < a.nsplit; s++) {
        const int64_t row_lo = (int64_t)s * a.rows_per_split;
        const int64_t row_hi = row_lo + a.rows_per_split < kp.N ? row_lo + a.rows_per_split : kp.N;
        // a trip of the workgroup covers 64 rows: wave w, group u of the trip, lane group g -> row 16 u + 4 w + g
        for (int64_t jb = row_lo + 4 * wave; jb < row_hi; jb += 64) {         // (wave-uniform: the MFMAs need every lane)
            double d0[4], d1[4], al[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t j = jb + 16 * u + g;
                const bool in = j < row_hi;
                al[u] = in ? a.alpha_[j] : 0.0;
                d0[u] = in && ok0 ? x0 - a.Xs[j * kp.dpad + r] : 0.0;
                d1[u] = 0.0;
                if (WIDE) d1[u] = in && ok1 ? x1 - a.Xs[j * kp.dpad + 16 + r] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                double r2 = d0[u] * d0[u];
                if (WIDE) r2 = fma(d1[u], d1[u], r2);
                r2 += __shfl_xor(r2, 1);
                r2 += __shfl_xor(r2, 2);
                r2 += __shfl_xor(r2, 4);
                r2 += __shfl_xor(r2, 8);
                double cq, cw;
                hess_weights<KID>(r2, al[u], &cq, &cw);
                T += cw;
                G0 = fma(cw, d0[u], G0);
                LL = __builtin_amdgcn_mfma_f64_16x16x4f64(cq * d0[u], d0[u], LL, 0, 0, 0);
                if (WIDE) {
                    G1 = fma(cw, d1[u], G1);
                    HL = __builtin_amdgcn_mfma_f64_16x16x4f64(cq * d1[u], d0[u], HL, 0, 0, 0);
                    HH = __builtin_amdgcn_mfma_f64_16x16x4f64(cq * d1[u], d1[u], HH, 0, 0, 0);
                }
            }
        }
    }
    // the four rows a lane group holds at a time: G and T summed over the groups, then everything to LDS per wave
    G0 += __shfl_down(G0, 32); G0 += __shfl_down(G0, 16);
    G1 += __shfl_down(G1, 32); G1 += __shfl_down(G1, 16);
    T += __shfl_down(T, 32); T += __shfl_down(T, 16);
    double* W = r2s + wave * HESS_WSTRIDE;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        W[q * 64 + lane] = LL[q];
        W[256 + q * 64 + lane] = HL[q];
        W[512 + q * 64 + lane] = HH[q];
    }
    if (lane < 16) { W[HESS_G_OFF + lane] = G0; W[HESS_G_OFF + 16 + lane] = G1; }
    if (lane == 0) W[HESS_T_OFF] = T;
    __syncthreads();
    auto comb = [&](int i) {
        return (r2s[i] + r2s[HESS_WSTRIDE + i]) + (r2s[2 * HESS_WSTRIDE + i] + r2s[3 * HESS_WSTRIDE + i]);
    };
    const double Tt = comb(HESS_T_OFF);
    const double sc = a.y_std * kp.C;
    // thread t holds element (m = g + 4 wave, n = r) of every tile: accumulator register `wave` of lane `lane`
    const int m = g + 4 * wave, n = r;
    double* Hp = H_out + p * d * d;
    const double fn = n < d ? ap.ls[n] * ap.span[n] : 1.0;
    if (m < d && n <= m) {
        const double fm = ap.ls[m] * ap.span[m];
        const double h = sc * (comb(t) + (m == n ? Tt : 0.0)) / (fm * fn);
        Hp[m * d + n] = h;
        Hp[n * d + m] = h;
    }
    if (WIDE && 16 + m < d) {
        const double fm = ap.ls[16 + m] * ap.span[16 + m];
        {
            const double h = sc * comb(256 + t) / (fm * fn);                    // (n < 16 < d)
            Hp[(16 + m) * d + n] = h;
            Hp[n * d + 16 + m] = h;
        }
        if (n <= m) {
            const double fn1 = ap.ls[16 + n] * ap.span[16 + n];
            const double h = sc * (comb(512 + t) + (m == n ? Tt : 0.0)) / (fm * fn1);
            Hp[(16 + m) * d + 16 + n] = h;
            Hp[(16 + n) * d + 16 + m] = h;
        }
    }
    if (t < d) g_out[p * d + t] = sc * comb(HESS_G_OFF + t) / (ap.ls[t] * ap.span[t]);
    if (t == 0) y_out[p] = y;
}

extern "C" {

int gpry_hessian_mean(gpry_ctx* ctx, const double* X, int64_t npts, double* y_out, double* g_out, double* H_out,
                      double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_hessian_mean: ctx is NULL");
    if (!X || !y_out || !g_out || !H_out) return gpry_fail(ctx, -1, "gpry_hessian_mean: NULL argument");
    if (npts < 1 || npts > 0x7fffffffll) return gpry_fail(ctx, -1, "gpry_hessian_mean: npts = %lld", (long long)npts);
    GPRY_TRY(require_model(ctx, true));
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "gpry_hessian_mean: d = %d > %d", ctx->d, GPRY_MAX_DIM);
    if (ctx->kernel_id == GPRY_MATERN12)
        return gpry_fail(ctx, -1, "gpry_hessian_mean: the mean of a Matern-1/2 model is not differentiable at the "
                                  "training rows; it has no Hessian");
    const int d = ctx->d;
    const int64_t n = npts;
    GPRY_TRY(check_points_finite(ctx, "gpry_hessian_mean", X, n));
    // (the mean needs no box: ns_args is handed the unit one)
    double lo[GPRY_MAX_DIM], hi[GPRY_MAX_DIM];
    for (int k = 0; k < GPRY_MAX_DIM; k++) { lo[k] = 0.0; hi[k] = 1.0; }
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_hessian_mean", lo, hi, 0, &a, &kp, &ap));
    NsStage st(ctx);
    const auto rX = st.in(X, n * d);
    const auto ry = st.out(y_out, n), rg = st.out(g_out, n * d), rH = st.out(H_out, n * d * d);
    GPRY_TRY(st.begin());
#define HS(DP, KID) \
    hipLaunchKernelGGL((hessian_kernel<DP, KID>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap, st.dev(rX), \
                       st.dev(ry), st.dev(rg), st.dev(rH))
    DISPATCH_DP_KID(d, ctx->kernel_id, HS)
#undef HS
    return st.end(device_ms);
}

}  // extern "C"
