// The derivative of the surrogate's latent predictive variance in the hyper-parameters at a batch of points: the kernels
// behind gpry_var_theta_grad.  What is done with it (the spread of sigma and of the LogExp acquisition over the thetas the
// data allow, the chance that two proposals swap rank) is host-side, in gpry_amd/hyper.py: hyper_acq_spread.
//
// theta = [log C, log l_1 .. log l_d (, log w)], p entries; K = C phi(r) + diag(noise + w), V = L^-1.  For a point x with
// the cross-kernel row k = k*(x), dk_a = dk / dlog l_a = C h(r) diff_a^2 (h as in theta_grad.hip; 0 at r = 0 for Matern 1/2),
// dK_a = dK / dlog l_a the same expression between training rows (zero diagonal), t = V k and q = K^-1 k = V^T t:
//   var(x) = y_std^2 (C + w - |t|^2)
//   G_0(x) = y_std^2 ((C - |t|^2) - sum_i (noise_i + w) q_i^2)                 log C
//   G_a(x) = y_std^2 sum_i q_i ((dK_a q)_i - 2 dk_ia)                          log l_a
//   G_w(x) = y_std^2 w (1 + |q|^2)                                             log w
// The log C entry uses q^T (C phi) q = q^T k - q^T diag(noise + w) q and is formed as written: C - 2 k^T q + q^T (C phi) q
// cancels to nothing next to a training point.
//
// Setup, once per call ("var_theta_grad_setup"): lml_hess_km_launch (lml_hessian.hip) writes the d matrices dK_a among the
// training rows as full zero-padded squares -- the pairs kernel of gpry_lml_hessian without its Hessian sums.
// Per panel of at most vg_panel(Np) points -- 4096 up to 1024 padded rows, 2048 up to 2048, 1024 above -- with the columns
// padded to a multiple of 128 by zero columns ("var_theta_grad"):
//   pv_panel_launch         K* (Np x cols), gpry_predict_thetas_var's panel at the context's own theta;
//   gemm_f64_launch         T = V K*     (NN, KM_A_LOWER: k up to the end of the row tile's diagonal tile);
//   gemm_f64_launch         Q = V^T T    (TN, KM_AT_LOWER: k from the row tile's first row on);
//   gemm_f64_launch         P_a = dK_a Q for the d length scales in ONE batched launch, a in grid.z (KM_FULL);
//   vg_sums_kernel          one workgroup per 64 points and slice of 128 training rows, lane = point.  Wave w walks the slice's
//                           rows w, w + 4, ... below N (a row's coordinates, noise and the 64 entries of T, Q and P_a are
//                           wave-uniform or contiguous); per row r^2 is the panel's fma chain over the coordinates in
//                           ascending order, then h, and |t|^2, |q|^2, sum (noise + w) q^2 and, per length scale,
//                           sum q (P_a - 2 dk_a) each take one fma.  The four waves are combined as (w0 + w1) + (w2 + w3);
//   vg_finish_kernel        per point: the slices' sums added in ascending order, then var and the row of G.
// Every element of an MFMA product is an accumulation chain of its own in k order, all shapes handed to the engine are
// multiples of 128 (its variant does not depend on the call), no product is split over k, and the sums walk the rows in
// slices and an order that are functions of N alone.  Hence var[i] and G[i, :] depend on the model and the point alone: not on
// npts, positions, the other points of a panel, the split of a batch over panels, chunks or calls, or the context.  A
// point whose k* underflows gives t = q = 0 exactly, and [y_std^2 C, 0 .., y_std^2 w].
//
// State: reads V, the scaled training rows, the noise vector and the affine map; writes the call scratch (CallScratch,
// common.h; held for the length of the call; doubles: d Np^2 for the dK_a, then with pc = min(vg_panel(Np), npts rounded up to
// 128) 3 Np pc for K*, T and Q, d Np pc for the products, (Np / 128) 35 pc for the slices' sums and the batch items) and the
// staging buffer ctx->dmc (the points and the outputs of one chunk of VG_CHUNK points).
#include "ns_common.h"
#include <algorithm>

#define VG_PC_MAX 4096                      // points per panel at the most (vg_panel)
#define VG_CHUNK 65536                      // points per upload
#define VG_MAX_NP 4096
#define VG_SLICE 128                        // training rows per workgroup of the sums: the slices are a function of Np alone
#define VG_EX GPRY_MAX_DIM                  // slot of |t|^2 in a slice's sums; |q|^2 and sum (noise + w) q^2 behind it
#define VG_NC (GPRY_MAX_DIM + 3)
static_assert(GPRY_VAR_THETA_GRAD_PANEL % 128 == 0 && VG_PC_MAX % GPRY_VAR_THETA_GRAD_PANEL == 0 && VG_CHUNK % VG_PC_MAX == 0,
              "panels are whole engine tiles inside a chunk");
// points per panel, a function of the model size alone: Np pc = 2^22, so that T = V K* and Q = V^T T hand the engine 256 tiles
// per launch at every size (Np / 128 x pc / 128), between GPRY_VAR_THETA_GRAD_PANEL and VG_PC_MAX
static inline int64_t vg_panel(int64_t Np) {
    return Np <= 1024 ? VG_PC_MAX : Np <= 2048 ? VG_PC_MAX / 2 : GPRY_VAR_THETA_GRAD_PANEL;
}

// the batch items of the engine launch P_a = dK_a Q, a = 0 .. d - 1 (offsets relative to Km / Q / P)
__global__ void vg_items_kernel(GemmBatchItem* __restrict__ items, int d, int64_t Np, int cols, int64_t ld) {
    const int k = threadIdx.x;
    if (k >= d) return;
    GemmBatchItem it;
    it.a_off = (int64_t)k * Np * Np; it.b_off = 0; it.c_off = (int64_t)k * Np * ld;
    it.M = (int)Np; it.N = cols; it.K = (int)Np; it.pad = 0;
    items[k] = it;
}

// grid (the panel's points in 64s, Np / VG_SLICE); 256 threads.  X: the panel's raw points (npts x d); Tm, Qm: Np x ld; Pm: d
// pieces of Np x ld.  part[slice][k][column]: the slice's sums, k < d the length scales, then VG_EX + 0 .. 2: |t|^2, |q|^2,
// sum (noise + w) q^2.
template <int DP, int KID>
__global__ __launch_bounds__(256) void vg_sums_kernel(const double* __restrict__ Xs, const double* __restrict__ noise, KernParams kp,
                                                      AffParams ap, const double* __restrict__ X, int64_t npts,
                                                      const double* __restrict__ Tm, const double* __restrict__ Qm,
                                                      const double* __restrict__ Pm, int64_t ld, int64_t Np,
                                                      double* __restrict__ part) {
    constexpr int NC = DP + 3;                      // the length scales, then |t|^2, |q|^2, sum (noise + w) q^2
    __shared__ double red[2 * NC * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = kp.d;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const bool live = c < npts;
    // this lane's point, scaled as the panel scales it
    double x[DP];
#pragma unroll
    for (int k = 0; k < DP; k++) {
        double v = 0.0;
        if (k < d && live) {
            v = X[c * d + k];
            if (kp.has_aff) v = (v - ap.lo[k]) / ap.span[k];
            v = v / ap.ls[k];
        }
        x[k] = v;
    }
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) acc[k] = 0.0;
    const int64_t pstride = Np * ld;
    const int64_t row_lo = (int64_t)blockIdx.y * VG_SLICE;
    const int64_t row_hi = row_lo + VG_SLICE < kp.N ? row_lo + VG_SLICE : kp.N;
    for (int64_t i = row_lo + wave; i < row_hi; i += 4) {
        const double* __restrict__ xr = Xs + i * kp.dpad;
        const double q = Qm[i * ld + c], tv = Tm[i * ld + c];
        const double nw = noise[i] + kp.white;
        double df2[DP];
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DP; k++) {
            df2[k] = 0.0;
            if (k < d) {
                const double df = x[k] - xr[k];
                r2 = fma(df, df, r2);
                df2[k] = df * df;
            }
        }
        double kv;
        const double ch2 = -2.0 * (kp.C * corr_and_h<KID>(r2, &kv));
#pragma unroll
        for (int k = 0; k < DP; k++)
            if (k < d) acc[k] = fma(q, fma(ch2, df2[k], Pm[(int64_t)k * pstride + i * ld + c]), acc[k]);
        acc[DP] = fma(tv, tv, acc[DP]);
        acc[DP + 1] = fma(q, q, acc[DP + 1]);
        acc[DP + 2] = fma(nw, q * q, acc[DP + 2]);
    }
    // (w0 + w1) + (w2 + w3): the odd waves hand theirs over, then wave 2 its sum
    double* mine = red + (wave >> 1) * NC * 64;
    if (wave & 1) {
#pragma unroll
        for (int k = 0; k < NC; k++) mine[k * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (!(wave & 1)) {
#pragma unroll
        for (int k = 0; k < NC; k++) acc[k] += mine[k * 64 + lane];
    }
    __syncthreads();
    if (wave == 2) {
#pragma unroll
        for (int k = 0; k < NC; k++) red[k * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (wave != 0) return;
    double* __restrict__ out = part + (int64_t)blockIdx.y * VG_NC * ld + c;
#pragma unroll
    for (int k = 0; k < DP; k++)
        if (k < d) out[(int64_t)k * ld] = acc[k] + red[k * 64 + lane];
#pragma unroll
    for (int e = 0; e < 3; e++) out[(int64_t)(VG_EX + e) * ld] = acc[DP + e] + red[(DP + e) * 64 + lane];
}

// grid: the panel's points in 256s; 256 threads, one point each: the slices' sums added in ascending order, then var and the
// row of G
__global__ __launch_bounds__(256) void vg_finish_kernel(const double* __restrict__ part, int nslice, int64_t ld, int64_t npts,
                                                        KernParams kp, double ys2, double* __restrict__ var_out,
                                                        double* __restrict__ G_out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= npts) return;
    const int d = kp.d, np = d + 1 + kp.white_on;
    auto total = [&](int k) {
        double v = 0.0;
        for (int s = 0; s < nslice; s++) v += part[((int64_t)s * VG_NC + k) * ld + c];
        return v;
    };
    double* Gp = G_out + c * np;
    const double ss = total(VG_EX);
    Gp[0] = ys2 * ((kp.C - ss) - total(VG_EX + 2));
    for (int k = 0; k < d; k++) Gp[1 + k] = ys2 * total(k);
    if (kp.white_on) Gp[1 + d] = ys2 * (kp.white * (1.0 + total(VG_EX + 1)));
    if (var_out) var_out[c] = ys2 * ((kp.C + kp.white) - ss);
}

extern "C" {

int64_t gpry_var_theta_grad_panel(gpry_ctx* ctx) { return vg_panel(ctx ? ctx->Np : VG_MAX_NP); }

int gpry_var_theta_grad(gpry_ctx* ctx, const double* X, int64_t npts, double* var_out, double* G_out, double* device_ms) {
    const char* who = "gpry_var_theta_grad";
    if (!ctx) return gpry_fail(nullptr, -1, "%s: ctx is NULL", who);
    GPRY_TRY(serve_stop(ctx));
    if (!X || !G_out) return gpry_fail(ctx, -1, "%s: NULL argument", who);
    if (npts < 1) return gpry_fail(ctx, -1, "%s: npts = %lld", who, (long long)npts);
    if (ctx->N <= 0 || !ctx->have_theta || !ctx->factor_valid)
        return gpry_fail(ctx, -1, "%s: the context holds no valid factor (call gpry_factorize)", who);
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "%s: d = %d > %d", who, ctx->d, GPRY_MAX_DIM);
    const int d = ctx->d, np = ctx_ntheta(ctx);
    const int64_t N = ctx->N, Np = ctx->Np;
    if (Np > VG_MAX_NP)
        return gpry_fail(ctx, -1, "%s: %lld padded rows exceed the limit of %d", who, (long long)Np, VG_MAX_NP);
    GPRY_TRY(check_points_finite(ctx, who, X, npts));
    GPRY_TRY(check_x_affine(ctx, who));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GPRY_TRY(ensure_pred_xs(ctx));
    const int64_t pc = vg_panel(Np), pcw = std::min<int64_t>(pc, round_up(npts, 128));
    const int64_t sq = Np * Np, pan = Np * pcw;
    const int nslice = (int)(Np / VG_SLICE);
    // The call scratch: the d matrices dK_a, the panel K*, T, Q, the d products of a panel, the slices' sums, the batch items
    // of the product.  lml_hess_km_launch and pv_panel_launch take their buffers from here and claim nothing; the points and
    // outputs of a chunk stage through dmc (NsStage), which is no part of it.  Every launch is on ctx->stream, drained by the
    // last stg.end().
    CallScratch cs(ctx, who);
    const auto rKm = cs.take<double>((int64_t)d * sq), rKst = cs.take<double>(pan), rT = cs.take<double>(pan), rQ = cs.take<double>(pan),
               rP = cs.take<double>((int64_t)d * pan), rpart = cs.take<double>((int64_t)nslice * VG_NC * pcw);
    const auto ritems = cs.take<GemmBatchItem>(GPRY_MAX_DIM);
    GPRY_TRY(cs.claim());
    double *Km = cs.at(rKm), *Kst = cs.at(rKst), *Tm = cs.at(rT), *Qm = cs.at(rQ), *Pm = cs.at(rP), *part = cs.at(rpart);
    GemmBatchItem* items = cs.at(ritems);
    const KernParams kp = make_kp(ctx);
    const AffParams ap = make_ap(ctx, kp.has_aff);
    const double ys2 = ctx->tf.y_std * ctx->tf.y_std;
    hipStream_t st = ctx->stream;
    double ms_total = 0.0;
    {
        NsTimer tm;
        GPRY_TRY(ns_begin(ctx, &tm));
        {
            StageScope s(ctx, "var_theta_grad_setup");
            GPRY_TRY(lml_hess_km_launch(ctx, Km));
        }
        double ms = 0.0;
        GPRY_TRY(ns_end(ctx, &tm, &ms));
        ms_total += ms;
    }
    for (int64_t c0 = 0; c0 < npts; c0 += VG_CHUNK) {
        const int64_t n = std::min<int64_t>(VG_CHUNK, npts - c0);
        NsStage stg(ctx);
        const auto rX = stg.in(X + c0 * d, n * d);
        const auto rv = stg.out(var_out ? var_out + c0 : nullptr, n), rG = stg.out(G_out + c0 * np, n * np);
        GPRY_TRY(stg.begin());
        const double* dX = stg.dev(rX);
        for (int64_t p0 = 0; p0 < n; p0 += pc) {
            const int64_t m = std::min<int64_t>(pc, n - p0), cols = round_up(m, 128);
            StageScope s(ctx, "var_theta_grad");
            {
                StageScope sp(ctx, "var_theta_grad_panel");
                GPRY_TRY(pv_panel_launch(ctx, dX + p0 * d, m, cols, Kst, pcw));
            }
            {
                StageScope sc(ctx, "var_theta_grad_solve");
                GemmArgs g = {};
                g.A = ctx->dV; g.lda = Np; g.B = Kst; g.ldb = pcw; g.C = Tm; g.ldc = pcw;
                g.M = (int)Np; g.N = (int)cols; g.K = (int)Np; g.kmode = KM_A_LOWER; g.tile_map = TM_ROWMAJOR;
                GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
                g.B = Tm; g.C = Qm; g.kmode = KM_AT_LOWER;
                GPRY_TRY(gemm_f64_launch(ctx, g, true, false, EPI_STORE));
            }
            {
                StageScope sc(ctx, "var_theta_grad_products");
                hipLaunchKernelGGL(vg_items_kernel, dim3(1), dim3(64), 0, st, items, d, Np, (int)cols, pcw);
                HIP_TRY(ctx, hipGetLastError());
                GemmArgs g = {};
                g.A = Km; g.lda = Np; g.B = Qm; g.ldb = pcw; g.C = Pm; g.ldc = pcw;
                g.M = (int)Np; g.N = (int)cols; g.K = (int)Np; g.kmode = KM_FULL; g.tile_map = TM_ROWMAJOR;
                g.batch = items; g.n_batch = d; g.dma_ok = 1;
                GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
            }
            {
                StageScope sf(ctx, "var_theta_grad_finish");
                double* dvar = stg.dev(rv);
#define VGF(DP, KID) \
    hipLaunchKernelGGL((vg_sums_kernel<DP, KID>), dim3((unsigned)((m + 63) / 64), (unsigned)nslice), dim3(256), 0, st, ctx->dXs, \
                       ctx->dnoise, kp, ap, dX + p0 * d, m, Tm, Qm, Pm, pcw, Np, part)
                DISPATCH_DP_KID(d, ctx->kernel_id, VGF)
#undef VGF
                hipLaunchKernelGGL(vg_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, part, nslice, pcw, m, kp, ys2,
                                   dvar ? dvar + p0 : nullptr, stg.dev(rG) + p0 * np);
                HIP_TRY(ctx, hipGetLastError());
            }
        }
        double ms = 0.0;
        GPRY_TRY(stg.end(&ms));
        ms_total += ms;
    }
    (void)N;
    if (device_ms) *device_ms = ms_total;
    return 0;
}

}  // extern "C"
