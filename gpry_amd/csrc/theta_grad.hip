// The derivative of the surrogate's posterior mean in the hyper-parameters at a batch of points: the kernels behind
// gpry_mean_theta_grad.  What is done with it (the part of a prediction's error bar that comes from theta, the first-order
// reweighting of a Monte Carlo sample under draws of theta) is host-side, in gpry_amd/hyper.py: hyper_spread.
//
// theta = [log C, log l_1 .. log l_d (, log w)], p entries, transformed units; K = C phi(r) + diag(noise + w),
// alpha_ = K^-1 y_, V = L^-1.  With diff_ia = x_a / l_a - X_ia / l_a (the kernel's coordinates, Xs holds the scaled rows),
// r_i = |diff_i|, k_i = C phi(r_i) and h(r) = -phi'(r) / r (minus the radial factor w(r) of mean_grad.h; d k_i / d log l_a =
// C h(r_i) diff_ia^2; Matern 1/2: h = e^-r / r, and h diff^2 -> 0 at r = 0):
//   U_0 = (noise + w) o alpha_,   U_a[i] = C sum_m h(r_im) diff_ima^2 alpha_m = (dK / dlog l_a) alpha_,   U_w = w alpha_
//   W = K^-1 U = V^T (V U)                                                          (N x p, once per call)
//   G_0(x) = y_std sum_i k_i W_i0
//   G_a(x) = y_std sum_i (C alpha_i h(r_i) diff_ia^2 - k_i W_ia)
//   G_w(x) = -y_std sum_i k_i W_iw
// of the unclipped, ungated mean.  The log C entry is formed as k*^T K^-1 (D alpha_), not as mean - k*^T K^-1 K_0 alpha_: it is
// about 1e-3 of the others and the difference form cancels two O(1) numbers to get it.
//
// tg_point_sums is the pass over the training rows of ONE point by one 256-thread workgroup, in hessian.hip's layout: a wave
// walks its rows four at a time, lane (g = lane >> 4, r = lane & 15) holds coordinate r (and 16 + r for d > 16) of row g of
// the four, r^2 of a row is summed over its 16 lanes.  Both terms of G_a are lane-local; the log C and log w entries ride in
// lanes r = 0 and r = 1.  The slices of the one-point path are walked in slice order, the lane groups are added as
// (g0 + g2) + (g1 + g3), the four waves through LDS as (w0 + w1) + (w2 + w3).  The columns U_a are its first sum at the
// training rows: the setup calls the same function without the W term.
//
// Setup, three launches: tg_rhs_kernel (U, one workgroup per training row), tg_vu_kernel (T = V U, one wave per row, the
// lanes walk the row 64 columns at a time, fixed butterfly), tg_vtt_kernel (W = V^T T, one workgroup per 64 columns, the
// waves take every fourth row, (w0 + w1) + (w2 + w3)).  Every sum has a fixed order: W's bits depend on the model alone.
// The call scratch (CallScratch, common.h; 2 Np TG_LD doubles, held for the length of the call): U column-major and, once
// T is formed, W row-major in its place; T row-major.
// Columns: the length scales at 0 .. 31, log C at TG_EX, log w at TG_EX + 1.  W is recomputed by every call.
#include "ns_common.h"

#define TG_LD 40            // row stride of T and W, column count of U
#define TG_EX 32            // slot of log C; log w at TG_EX + 1
#define TG_SUMS 80          // sums of a point: first term (32), k W term (32), log C / log w (16, two used)
#define TG_CHUNK 65536      // points per launch

__host__ __device__ constexpr int tg_col(int c, int NL) { return c < NL ? c : TG_EX + (c - NL); }

// The sums of one point over the training rows.  x0 / x1: this lane's scaled coordinates r and 16 + r of the point (0 where
// there is none).  lds: 4 * TG_SUMS doubles.  out (LDS, TG_SUMS doubles, valid after the call in every thread):
//   out[a]      = sum_i C alpha_i h(r_i) diff_ia^2            a < 32
//   out[32 + a] = sum_i k_i W_ia                              (WITHW)
//   out[64 + e] = sum_i k_i W_i,TG_EX + e                     e = 0, 1 (WITHW)
template <bool WIDE, int KID, bool WITHW>
__device__ __forceinline__ void tg_point_sums(double x0, double x1, bool ok0, bool ok1, const NsArgs& a, const KernParams& kp,
                                              const double* __restrict__ W, double* lds, double* out) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    double A0 = 0.0, A1 = 0.0, B0 = 0.0, B1 = 0.0, E = 0.0;
    for (int s = 0; s < a.nsplit; s++) {
        const int64_t row_lo = (int64_t)s * a.rows_per_split;
        const int64_t row_hi = row_lo + a.rows_per_split < kp.N ? row_lo + a.rows_per_split : kp.N;
        // a trip of the workgroup covers 64 rows: wave w, group u of the trip, lane group g -> row 16 u + 4 w + g
        for (int64_t jb = row_lo + 4 * wave; jb < row_hi; jb += 64) {         // (wave-uniform: the cross-lane sums need every lane)
            double d0[4], d1[4], al[4], w0[4], w1[4], we[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t j = jb + 16 * u + g;
                const bool in = j < row_hi;
                al[u] = in ? a.alpha_[j] : 0.0;
                d0[u] = in && ok0 ? x0 - a.Xs[j * kp.dpad + r] : 0.0;
                d1[u] = 0.0;
                if (WIDE) d1[u] = in && ok1 ? x1 - a.Xs[j * kp.dpad + 16 + r] : 0.0;
                w0[u] = 0.0; w1[u] = 0.0; we[u] = 0.0;
                if (WITHW) {
                    w0[u] = in ? W[j * TG_LD + r] : 0.0;
                    if (WIDE) w1[u] = in ? W[j * TG_LD + 16 + r] : 0.0;
                    we[u] = in ? W[j * TG_LD + TG_EX + (r & 1)] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                double r2 = d0[u] * d0[u];
                if (WIDE) r2 = fma(d1[u], d1[u], r2);
                r2 += __shfl_xor(r2, 1);
                r2 += __shfl_xor(r2, 2);
                r2 += __shfl_xor(r2, 4);
                r2 += __shfl_xor(r2, 8);
                double kv;
                const double h = corr_and_h<KID>(r2, &kv);
                const double ca = kp.C * (al[u] * h), ck = kp.C * kv;
                A0 = fma(ca, d0[u] * d0[u], A0);
                if (WIDE) A1 = fma(ca, d1[u] * d1[u], A1);
                if (WITHW) {
                    B0 = fma(ck, w0[u], B0);
                    if (WIDE) B1 = fma(ck, w1[u], B1);
                    E = fma(ck, we[u], E);
                }
            }
        }
    }
    // the four rows a lane group holds at a time, then the waves through LDS
    A0 += __shfl_down(A0, 32); A0 += __shfl_down(A0, 16);
    A1 += __shfl_down(A1, 32); A1 += __shfl_down(A1, 16);
    B0 += __shfl_down(B0, 32); B0 += __shfl_down(B0, 16);
    B1 += __shfl_down(B1, 32); B1 += __shfl_down(B1, 16);
    E += __shfl_down(E, 32); E += __shfl_down(E, 16);
    if (lane < 16) {
        double* L = lds + wave * TG_SUMS;
        L[lane] = A0; L[16 + lane] = A1; L[32 + lane] = B0; L[48 + lane] = B1; L[64 + lane] = E;
    }
    __syncthreads();
    if (t < TG_SUMS) out[t] = (lds[t] + lds[TG_SUMS + t]) + (lds[2 * TG_SUMS + t] + lds[3 * TG_SUMS + t]);
    __syncthreads();
}

// U, one workgroup per training row i: the length-scale columns from tg_point_sums at the row's own scaled coordinates,
// (noise_i + w) alpha_i and w alpha_i.  U is column-major, column c at U + c * Np; the NL + 2 columns the products read are
// written, zeros where the model has no such entry.
template <bool WIDE, int KID>
__global__ __launch_bounds__(256) void tg_rhs_kernel(NsArgs a, KernParams kp, const double* __restrict__ noise, int64_t Np,
                                                     double* __restrict__ U) {
    __shared__ double lds[4 * TG_SUMS];
    __shared__ double out[TG_SUMS];
    const int t = threadIdx.x, r = t & 15;
    const int64_t i = blockIdx.x;
    const bool ok0 = r < kp.d, ok1 = WIDE && 16 + r < kp.d;
    const double x0 = ok0 ? a.Xs[i * kp.dpad + r] : 0.0, x1 = ok1 ? a.Xs[i * kp.dpad + 16 + r] : 0.0;
    tg_point_sums<WIDE, KID, false>(x0, x1, ok0, ok1, a, kp, nullptr, lds, out);
    if (t < (WIDE ? 32 : 16)) U[(int64_t)t * Np + i] = t < kp.d ? out[t] : 0.0;
    if (t == 64) U[(int64_t)TG_EX * Np + i] = (noise[i] + kp.white) * a.alpha_[i];
    if (t == 65) U[(int64_t)(TG_EX + 1) * Np + i] = kp.white * a.alpha_[i];
}

// T = V U (V lower triangular, row-major; only its entries with column <= row < N are read).  One wave per row: the lanes
// walk the row's columns 64 at a time with one partial sum per column of U, added by a fixed butterfly.  T is row-major.
template <int NL>
__global__ __launch_bounds__(256) void tg_vu_kernel(const double* __restrict__ V, int64_t Np, int64_t N, const double* __restrict__ U,
                                                    double* __restrict__ T) {
    constexpr int NC = NL + 2;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                 // (the whole wave)
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
    for (int64_t c0 = 0; c0 <= i; c0 += 64) {
        const int64_t j = c0 + lane;
        const bool in = j <= i;
        const double v = in ? V[i * Np + j] : 0.0;
        const int64_t jj = in ? j : i;
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = fma(v, U[(int64_t)tg_col(c, NL) * Np + jj], acc[c]);
    }
    double mine = 0.0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        double v = acc[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == c) mine = v;
    }
    if (lane < NC) T[i * TG_LD + tg_col(lane, NL)] = mine;
}

// W = V^T T.  One workgroup per 64 columns j of V (lane = column: rows of V are read as whole lines), wave w takes the rows
// j0 + w, j0 + w + 4, ... below N; the four waves are combined as (w0 + w1) + (w2 + w3).  W is row-major.
template <int NL>
__global__ __launch_bounds__(256) void tg_vtt_kernel(const double* __restrict__ V, int64_t Np, int64_t N, const double* __restrict__ T,
                                                     double* __restrict__ W) {
    constexpr int NC = NL + 2;
    __shared__ double red[2 * NC * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j0 = (int64_t)blockIdx.x * 64, j = j0 + lane;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
#pragma unroll 2
    for (int64_t i = j0 + wave; i < N; i += 4) {
        const double v = j <= i ? V[i * Np + j] : 0.0;
        const double* __restrict__ Ti = T + i * TG_LD;
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = fma(v, Ti[tg_col(c, NL)], acc[c]);
    }
    // (w0 + w1) + (w2 + w3): the odd waves hand theirs over, then wave 2 its sum
    double* mine = red + (wave >> 1) * NC * 64;
    if (wave & 1) {
#pragma unroll
        for (int c = 0; c < NC; c++) mine[c * 64 + lane] = acc[c];
    }
    __syncthreads();
    if (!(wave & 1)) {
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] += mine[c * 64 + lane];
    }
    __syncthreads();
    if (wave == 2) {
#pragma unroll
        for (int c = 0; c < NC; c++) red[c * 64 + lane] = acc[c];
    }
    __syncthreads();
    if (wave == 0 && j < N) {
#pragma unroll
        for (int c = 0; c < NC; c++) W[j * TG_LD + tg_col(c, NL)] = acc[c] + red[c * 64 + lane];
    }
}

// One workgroup per point: y is ns_eval of the point (gpry_predict(x[None]) bit for bit), G its row of p entries.
template <int DP, int KID>
__global__ __launch_bounds__(256) void theta_grad_kernel(NsArgs a, KernParams kp, AffParams ap, const double* __restrict__ X,
                                                         const double* __restrict__ W, double* __restrict__ y_out,
                                                         double* __restrict__ G_out) {
    constexpr bool WIDE = DP > 16;
    __shared__ double r2s[MEAN_SLICE_CH];        // ns_eval's rows of r^2, then the waves' partial sums
    __shared__ double red[256];
    __shared__ double s_x[GPRY_MAX_DIM];
    __shared__ double s_y;
    static_assert(5 * TG_SUMS <= MEAN_SLICE_CH, "the waves' partial sums reuse r2s");
    const int t = threadIdx.x, r = t & 15, d = kp.d;
    const int64_t p = blockIdx.x;
    if (t < GPRY_MAX_DIM) s_x[t] = t < d ? X[p * d + t] : 0.0;
    __syncthreads();
    const double y = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);

    // this lane's scaled coordinates of the point (mean_slice's arithmetic)
    const bool ok0 = r < d, ok1 = WIDE && 16 + r < d;
    double x0 = 0.0, x1 = 0.0;
    if (ok0) { double v = s_x[r]; if (kp.has_aff) v = (v - ap.lo[r]) / ap.span[r]; x0 = v / ap.ls[r]; }
    if (ok1) { double v = s_x[16 + r]; if (kp.has_aff) v = (v - ap.lo[16 + r]) / ap.span[16 + r]; x1 = v / ap.ls[16 + r]; }
    double* out = r2s + 4 * TG_SUMS;
    tg_point_sums<WIDE, KID, true>(x0, x1, ok0, ok1, a, kp, W, r2s, out);
    const int np = d + 1 + kp.white_on;
    double* Gp = G_out + p * np;
    if (t < d) Gp[1 + t] = a.y_std * (out[t] - out[32 + t]);
    if (t == 64) Gp[0] = a.y_std * out[64];
    if (t == 65 && kp.white_on) Gp[1 + d] = -(a.y_std * out[65]);
    if (t == 0 && y_out) y_out[p] = y;
}

extern "C" {

int gpry_mean_theta_grad(gpry_ctx* ctx, const double* X, int64_t npts, double* y_out, double* G_out, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_mean_theta_grad: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    if (!X || !G_out) return gpry_fail(ctx, -1, "gpry_mean_theta_grad: NULL argument");
    if (npts < 1) return gpry_fail(ctx, -1, "gpry_mean_theta_grad: npts = %lld", (long long)npts);
    GPRY_TRY(require_model(ctx, true));
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "gpry_mean_theta_grad: d = %d > %d", ctx->d, GPRY_MAX_DIM);
    const int d = ctx->d, np = ctx_ntheta(ctx);
    GPRY_TRY(check_points_finite(ctx, "gpry_mean_theta_grad", X, npts));
    // (the mean needs no box: ns_args is handed the unit one)
    double lo[GPRY_MAX_DIM], hi[GPRY_MAX_DIM];
    for (int k = 0; k < GPRY_MAX_DIM; k++) { lo[k] = 0.0; hi[k] = 1.0; }
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_mean_theta_grad", lo, hi, 0, &a, &kp, &ap));
    const int64_t N = ctx->N, Np = ctx->Np;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the call scratch: U (and W in its place), T.  The point batches below stage through dmc (NsStage), which is no part
    // of it; every launch is on ctx->stream, drained by the last st.end().
    CallScratch cs(ctx, "gpry_mean_theta_grad");
    const auto rU = cs.take<double>(Np * TG_LD), rT = cs.take<double>(Np * TG_LD);
    GPRY_TRY(cs.claim());
    double *U = cs.at(rU), *T = cs.at(rT), *W = U;
    const bool wide = d > 16;
    double ms_total = 0.0;
    {
        NsTimer tm;
        GPRY_TRY(ns_begin(ctx, &tm));
        {
            StageScope s(ctx, "theta_grad_setup");
#define TGR2(WIDE, KID) hipLaunchKernelGGL((tg_rhs_kernel<WIDE, KID>), dim3((unsigned)N), dim3(256), 0, ctx->stream, a, kp, ctx->dnoise, Np, U)
#define TGR(KID) { if (wide) TGR2(true, KID); else TGR2(false, KID); }
            DISPATCH_KID(ctx->kernel_id, TGR)
#undef TGR
#undef TGR2
            if (wide) {
                hipLaunchKernelGGL(tg_vu_kernel<32>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, ctx->dV, Np, N, U, T);
                hipLaunchKernelGGL(tg_vtt_kernel<32>, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, ctx->stream, ctx->dV, Np, N, T, W);
            } else {
                hipLaunchKernelGGL(tg_vu_kernel<16>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, ctx->dV, Np, N, U, T);
                hipLaunchKernelGGL(tg_vtt_kernel<16>, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, ctx->stream, ctx->dV, Np, N, T, W);
            }
        }
        double ms = 0.0;
        GPRY_TRY(ns_end(ctx, &tm, &ms));
        ms_total += ms;
    }
    for (int64_t c0 = 0; c0 < npts; c0 += TG_CHUNK) {
        const int64_t n = npts - c0 < TG_CHUNK ? npts - c0 : TG_CHUNK;
        NsStage st(ctx);
        const auto rX = st.in(X + c0 * d, n * d);
        const auto ry = st.out(y_out ? y_out + c0 : nullptr, n), rG = st.out(G_out + c0 * np, n * np);
        GPRY_TRY(st.begin());
        {
            StageScope s(ctx, "theta_grad");
#define TG(DP, KID) \
    hipLaunchKernelGGL((theta_grad_kernel<DP, KID>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap, st.dev(rX), W, \
                       st.dev(ry), st.dev(rG))
            DISPATCH_DP_KID(d, ctx->kernel_id, TG)
#undef TG
        }
        double ms = 0.0;
        GPRY_TRY(st.end(&ms));
        ms_total += ms;
    }
    if (device_ms) *device_ms = ms_total;
    return 0;
}

}  // extern "C"
