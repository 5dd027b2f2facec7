// gpry_predict_thetas: the posterior mean at M points under B thetas in one call, without touching the model the context
// holds.  For theta b = [log C, log l_1 .. l_d (, log w)] and point x_i (raw coordinates where the affine map has an
// x-affine):
//   mean[b, i] = y_mean + y_std k_b(x_i)^T alpha_b,    alpha_b = (C_b phi_b + diag(noise + w_b))^-1 y_
// the unclipped, ungated mean in untransformed units (the quantity gpry_mean_theta_grad differentiates), and with it
// lml[b] and info[b] as gpry_lml(theta_b, want_grad = 0) returns them.  What hyper_spread(exact=True) of gpry_amd/hyper.py
// is made of: the exact reweighting of a Monte Carlo sample under draws of theta, one refactorisation per draw.
//
// Route: the thetas go through gpry_lml's value-only chain (lml_chain: build_factor, solve_alpha, logdet_and_quad) with all
// thetas of a chunk in grid.z (objective_batch_general, api.hip, always in the latency schedule), each theta in a scratch
// set of its own; predict_thetas_kernel then reads every set's scaled training rows, alpha_ and parameter row while the
// chunk is resident.  Where the batched chain is not available (Np above option "lml_batch", the rocSOLVER comparator,
// fewer than two sets fit, one theta, Np = 128) the thetas go one after another through the same chain in the context's
// own scratch, followed by the same kernel: the same bits.
//
// predict_thetas_kernel, grid (ceil(points / 4), 1, thetas), 256 threads: one workgroup evaluates four points of one theta
// with ns_eval_multi (ns_common.h), i.e. with mean_slice's arithmetic operation for operation -- the slices of the
// one-point path, the two scaled coordinates per lane ((x - lo) / span / l), the xor-shuffle sum of r^2, phase 2's groups
// (v0 + v1) + (v2 + v3), the one-barrier tree, the finish ns_rn(mu y_std) + y_mean -- on the theta's own scaled rows, alpha_
// and [C, l...] row, with the clip at +inf and no gates.  Every training row and alpha_ is loaded once per four points.
// A value therefore has the bits gpry_predict(x[None]) has on a context factorised at that theta with the clip off and
// no gates, and every summation order is a function of N alone: the bits of mean[b, i] depend on the model, theta_b and
// x_i, never on B, M, positions, chunking, the route or option "lml_batch_mb".  (A form with one point per lane, the
// training rows broadcast from LDS and one running sum per point runs the points four to five times as fast and was
// measured; its sums have another order than every other mean of this library, and where two weights of opposite sign
// and size 500 meet -- duplicated training rows -- it differs from them by 3e-13 of the mean.  It was not kept.)
//
// gpry_predict_thetas_var: the same call with the predictive variance beside the mean,
//   var[b, i] = y_std^2 ((C_b + w_b) - |V_b k_b(x_i)|^2),    V_b = L_b^-1,
// not clamped at 0 (gpry_predict_cov's diagonal).  The value-only chain leaves V_b in the theta's second N x N piece
// (solve_alpha needs it) and is finished with the third (T of the factor chain: every reader of it runs a chain of its
// own first), so that piece takes the cross-kernel panel of pv_panel_points(Np) points and, behind it, the partial
// sums.  Per panel of points, with the thetas of the chunk in grid.z:
//   pt_var_panel_kernel     K*_b (Np rows x the panel's columns, padded to 64): C_b corr_r2_fast(r^2), r^2 one fma
//                           chain over the coordinates in ascending order, the point scaled as the point kernel scales it
//                           ((x - lo) / span / l); rows from N on and columns beyond the panel's points are exact zeros;
//   gemm_f64_kernel         U = V_b K*_b by the project's FP64 MFMA engine (gemm_f64.hip) with KM_A_LOWER and the EPI_SUMSQ
//                           epilogue, the product of the sweep's register-staged contraction (sweep.hip: contract_sweep), row-major tiles:
//                           128 x 128 tiles, k ascending from 0 to the end of the row block's diagonal tile -- the tiles of V
//                           above the diagonal are never visited -- and the column sums of squares taken in the epilogue
//                           into one partial sum per row block and point; U never goes to HBM.  The engine takes the
//                           theta from grid.z (gemm_fill_batch) and leaves a theta without a factor alone (info);
//   pt_var_finish_kernel    the row blocks' partial sums added in ascending order, then y_std^2 ((C_b + w_b) - ss).
// Each column of an MFMA tile is an accumulation chain of its own and every order above is a function of Np alone, so
// the bits of var[b, i] depend on the model, theta_b and x_i, never on B, M, positions, the other points of the tile,
// chunking, the route or option "lml_batch_mb"; a point whose k underflows gives y_std^2 (C_b + w_b) exactly.
#include "ns_common.h"

#define PT_R 4              // points per workgroup
#define PT_CHUNK 65536      // points per launch
#define PT_MAXB 96          // thetas per chain at the most (objective_batch_general's chunk)
#define PV_BM 128           // rows of V per row block of the contraction (the engine's tile)
#define PV_BN 64            // what a panel's columns are padded to (the panel kernel's tile; the engine guards its columns by eights)
#define PV_LDX (GPRY_MAX_DIM + 1)

template <int DP, int KID>
__global__ __launch_bounds__(256) void predict_thetas_kernel(NsArgs a, KernParams kp, AffParams ap, const double* __restrict__ bpar,
                                                             int64_t bstride, const double* __restrict__ X, int64_t npts,
                                                             double* __restrict__ out, int64_t ldo) {
    __shared__ double r2s[PT_R * MEAN_MULTI_CH];
    __shared__ double s_x[PT_R * GPRY_MAX_DIM];
    __shared__ double s_y[PT_R];
    __shared__ AffParams s_ap;
    // batched launch (gpry_ctx::bn): the buffers and the parameter row of theta blockIdx.z
    const int z = (int)blockIdx.z, t = threadIdx.x, d = kp.d;
    a.Xs = bset(a.Xs, z, bstride);
    a.alpha_ = bset(a.alpha_, z, bstride);
    const double* __restrict__ par = bpar ? bset(bpar, z, bstride) : nullptr;
    if (par) kp.C = par[0];
    if (t < GPRY_MAX_DIM) {
        s_ap.ls[t] = par ? par[1 + t] : ap.ls[t];          // (unused slots of a parameter row are 1, as make_ap's)
        s_ap.lo[t] = ap.lo[t]; s_ap.span[t] = ap.span[t];
    }
    const int64_t p0 = (int64_t)blockIdx.x * PT_R;
    if (t < PT_R * GPRY_MAX_DIM) {
        const int p = t / GPRY_MAX_DIM, k = t - p * GPRY_MAX_DIM;
        s_x[t] = (p0 + p < npts && k < d) ? X[(p0 + p) * d + k] : 0.0;
    }
    __syncthreads();
    unsigned mask = 0;
#pragma unroll
    for (int p = 0; p < PT_R; p++) mask |= p0 + p < npts ? 1u << p : 0u;
    double y[PT_R];
#pragma unroll
    for (int p = 0; p < PT_R; p++) y[p] = 0.0;
    ns_eval_multi<DP, KID, PT_R>(s_x, mask, a, kp, s_ap, r2s, s_y, y);
    if (t == 0) {
#pragma unroll
        for (int p = 0; p < PT_R; p++)
            if (mask >> p & 1u) out[(int64_t)z * ldo + p0 + p] = y[p];
    }
}

template <int KID>
__global__ __launch_bounds__(256) void pt_var_panel_kernel(const double* __restrict__ Xs_, int64_t N, int d, int dpad, int has_aff,
                                                           AffParams ap, double C, const double* __restrict__ bpar, int64_t bstride,
                                                           const double* __restrict__ X, int64_t npts, double* __restrict__ Kst_,
                                                           int64_t ldk) {
    __shared__ double s_p[PV_BN * PV_LDX];      // the tile's points, scaled
    __shared__ double s_r[64 * PV_LDX];         // 64 scaled training rows
    const int z = (int)blockIdx.z, t = threadIdx.x;
    const double* __restrict__ Xs = bset(Xs_, z, bstride);
    double* __restrict__ Kst = bset(Kst_, z, bstride);
    const double* __restrict__ par = bpar ? bset(bpar, z, bstride) : nullptr;
    if (par) C = par[0];
    const int64_t c0 = (int64_t)blockIdx.x * PV_BN, r0 = (int64_t)blockIdx.y * 64;
    for (int e = t; e < PV_BN * d; e += 256) {
        const int p = e / d, k = e - p * d;
        double v = 0.0;
        if (c0 + p < npts) {
            v = X[(c0 + p) * d + k];
            if (has_aff) v = (v - ap.lo[k]) / ap.span[k];
            v = v / (par ? par[1 + k] : ap.ls[k]);
        }
        s_p[p * PV_LDX + k] = v;
        s_r[p * PV_LDX + k] = Xs[(r0 + p) * dpad + k];          // (r0 + p < Np: the grid covers the padded rows)
    }
    __syncthreads();
    const int col = t & 63, rg = t >> 6;
    for (int i = 0; i < 16; i++) {
        const int row = rg * 16 + i;
        double r2 = 0.0;
        for (int k = 0; k < d; k++) {
            const double df = s_p[col * PV_LDX + k] - s_r[row * PV_LDX + k];
            r2 = fma(df, df, r2);
        }
        const double v = (r0 + row < N && c0 + col < npts) ? C * corr_r2_fast<KID>(r2) : 0.0;
        Kst[(r0 + row) * ldk + c0 + col] = v;
    }
}

int pv_panel_launch(gpry_ctx* ctx, const double* dX, int64_t npts, int64_t cols, double* Kst, int64_t ldk) {
    const KernParams kp = make_kp(ctx);
    const AffParams ap = make_ap(ctx, kp.has_aff);
#define PV(KID) \
    hipLaunchKernelGGL((pt_var_panel_kernel<KID>), dim3((unsigned)(cols / PV_BN), (unsigned)(ctx->Np / 64), 1), dim3(256), 0, ctx->stream, \
                       ctx->dXs, ctx->N, ctx->d, ctx->dpad, kp.has_aff, ap, kp.C, (const double*)nullptr, (int64_t)0, dX, npts, Kst, ldk)
    DISPATCH_KID(ctx->kernel_id, PV)
#undef PV
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void pt_var_finish_kernel(const double* __restrict__ part_, int64_t ldk, int nrb, double prior,
                                                            const double* __restrict__ bpar, int64_t bstride, double ys2, int64_t n,
                                                            double* __restrict__ out, int64_t ldo) {
    const int z = (int)blockIdx.z;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const double* __restrict__ part = bset(part_, z, bstride);
    if (bpar) { const double* par = bset(bpar, z, bstride); prior = par[0] + par[GPRY_BPAR_WHITE]; }
    double ss = 0.0;
    for (int ti = 0; ti < nrb; ti++) ss += part[(int64_t)ti * ldk + c];
    out[(int64_t)z * ldo + c] = ys2 * (prior - ss);
}

namespace {

// the call in flight: the chain below is handed to objective_batch_general as a plain function and finds the points, the
// output and how far the thetas have come here
struct PtCall {
    const double* dX = nullptr;     // the M x d points on the device
    double* dout = nullptr;         // PT_MAXB x ldo means of the chunk in flight
    int64_t M = 0, ldo = 0;
    double* mean = nullptr;         // the caller's B x M
    double* dvar = nullptr;         // PT_MAXB x ldo variances of the chunk in flight (NULL: the mean alone)
    double* var = nullptr;          // the caller's B x M
    int64_t done = 0;               // thetas whose rows have been queued
};
thread_local PtCall* g_pt = nullptr;

// points per panel: the third N x N piece of a scratch set holds the Np x pc panel and the Np / 128 x pc partial
// sums behind it (a function of Np alone; 64 at Np = 128)
int64_t pv_panel_points(int64_t Np) { return Np * Np / (Np + Np / PV_BM) / PV_BN * PV_BN; }

// var of the ctx->bn thetas the chain has just served at points [c0, c0 + n) of the call, into c->dvar
int pt_var_chunk(gpry_ctx* ctx, const PtCall* c, const KernParams& kp, const AffParams& ap, int64_t c0, int64_t n) {
    StageScope s(ctx, "predict_thetas_var");
    const int64_t Np = ctx->Np, pc = pv_panel_points(Np);
    const int d = ctx->d, nrb = (int)(Np / PV_BM);
    const unsigned bn = (unsigned)ctx->bn;
    double* Kst = ctx->dW3;                 // free behind the value-only chain
    double* part = ctx->dW3 + Np * pc;
    const double ys2 = ctx->tf.y_std * ctx->tf.y_std;
    for (int64_t p0 = 0; p0 < n; p0 += pc) {
        const int64_t np = n - p0 < pc ? n - p0 : pc;
        const unsigned nct = (unsigned)((np + PV_BN - 1) / PV_BN);
#define PV(KID) \
    hipLaunchKernelGGL((pt_var_panel_kernel<KID>), dim3(nct, (unsigned)(Np / 64), bn), dim3(256), 0, ctx->stream, ctx->dXs, ctx->N, d, \
                       ctx->dpad, kp.has_aff, ap, kp.C, ctx->bpar, ctx->bstride, c->dX + (c0 + p0) * d, np, Kst, pc)
        DISPATCH_KID(ctx->kernel_id, PV)
#undef PV
        {
            StageScope sc(ctx, "predict_thetas_contract");
            GemmArgs g = {};
            g.A = ctx->dW2; g.lda = Np; g.B = Kst; g.ldb = pc; g.C = part; g.ldc = pc;
            g.M = (int)Np; g.N = (int)(nct * PV_BN); g.K = (int)Np;
            // (row-major tiles, as joint.hip's U = V K*^T: the sweep's super-tile map puts a panel of at most 64 tiles on one XCD)
            g.kmode = KM_A_LOWER; g.tile_map = TM_ROWMAJOR;
            g.info = ctx->dinfo;
            GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_SUMSQ));
        }
        hipLaunchKernelGGL(pt_var_finish_kernel, dim3((unsigned)((np + 255) / 256), 1, bn), dim3(256), 0, ctx->stream, part, pc, nrb,
                           ctx_prior_var(ctx), ctx->bpar, ctx->bstride, ys2, np, c->dvar + p0, c->ldo);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// gpry_lml's value-only chain, then the means of the ctx->bn thetas it served at all points, chunk of points by chunk
int pt_chain(gpry_ctx* ctx, int /*want_grad*/, double* dres) {
    PtCall* c = g_pt;
    if (!c) return gpry_fail(ctx, -1, "predict_thetas: no call in flight");
    if (ctx->bn > PT_MAXB) return gpry_fail(ctx, -1, "predict_thetas: %d thetas in one chain, the output holds %d", ctx->bn, PT_MAXB);
    GPRY_TRY(lml_chain(ctx, 0, dres));
    const KernParams kp = make_kp(ctx);
    const AffParams ap = make_ap(ctx, kp.has_aff);
    const int d = ctx->d;
    // ns_args' slices of the one-point path -- without its ensure_pred_xs: the rows here are the chain's own
    NsArgs a = {};
    a.Xs = ctx->dXs; a.alpha_ = ctx->dvec + ctx->Np;         // alpha_ of the chain
    a.nsplit = (int)(ctx->N / 1024);
    if (a.nsplit < 1) a.nsplit = 1;
    if (a.nsplit > 8) a.nsplit = 8;
    a.rows_per_split = round_up((ctx->N + a.nsplit - 1) / a.nsplit, 32);
    a.gates = 0;
    a.y_std = ctx->tf.y_std; a.y_mean = ctx->tf.y_mean; a.clip_hi = INFINITY;
    for (int k = 0; k < GPRY_MAX_DIM; k++) a.hi[k] = 1.0;
    for (int64_t c0 = 0; c0 < c->M; c0 += PT_CHUNK) {
        const int64_t n = c->M - c0 < PT_CHUNK ? c->M - c0 : PT_CHUNK;
        {
            StageScope s(ctx, "predict_thetas_mean");
            const dim3 grid((unsigned)((n + PT_R - 1) / PT_R), 1, (unsigned)ctx->bn);
#define PT(DP, KID) \
    hipLaunchKernelGGL((predict_thetas_kernel<DP, KID>), grid, dim3(256), 0, ctx->stream, a, kp, ap, ctx->bpar, ctx->bstride, \
                       c->dX + c0 * d, n, c->dout, c->ldo)
            DISPATCH_DP_KID(d, ctx->kernel_id, PT)
#undef PT
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpy2DAsync(c->mean + c->done * c->M + c0, sizeof(double) * c->M, c->dout, sizeof(double) * c->ldo,
                                      sizeof(double) * n, (size_t)ctx->bn, hipMemcpyDeviceToHost, ctx->stream));
        if (c->dvar) {
            GPRY_TRY(pt_var_chunk(ctx, c, kp, ap, c0, n));
            HIP_TRY(ctx, hipMemcpy2DAsync(c->var + c->done * c->M + c0, sizeof(double) * c->M, c->dvar, sizeof(double) * c->ldo,
                                          sizeof(double) * n, (size_t)ctx->bn, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    c->done += ctx->bn;
    return 0;
}

}  // namespace

namespace {

// both entry points: var == NULL is gpry_predict_thetas
int pt_run(gpry_ctx* ctx, const double* thetas, int64_t B, const double* X, int64_t M, double* mean, double* var, double* lml,
           int* info, double* device_ms) {
    if (!thetas || !X || !mean) return gpry_fail(ctx, -1, "predict_thetas: thetas, X and mean must not be NULL");
    if (B < 1 || M < 1) return gpry_fail(ctx, -1, "predict_thetas: B = %lld thetas, M = %lld points", (long long)B, (long long)M);
    if (ctx->N > 0 && !ctx->have_theta) return gpry_fail(ctx, -1, "predict_thetas: no kernel id (call gpry_set_theta)");
    GPRY_TRY(objective_entry(ctx, "predict_thetas", thetas, B));
    const int d = ctx->d, w = ctx_ntheta(ctx);
    GPRY_TRY(check_points_finite(ctx, "predict_thetas", X, M));
    GPRY_TRY(check_x_affine(ctx, "predict_thetas"));
    std::vector<double> vlml((size_t)B, 0.0);
    std::vector<int> vinfo((size_t)B, 0);

    // the points, once per call, and the means of one chunk of thetas and points: the samplers' staging buffer
    PtCall call;
    call.M = M; call.ldo = M < PT_CHUNK ? M : PT_CHUNK; call.mean = mean; call.var = var;
    const int64_t xbytes = round_up((int64_t)sizeof(double) * M * d, 256);
    const int64_t maxb = B < PT_MAXB ? B : PT_MAXB;
    const int64_t obytes = round_up((int64_t)sizeof(double) * maxb * call.ldo, 256);        // (used with var alone)
    GPRY_TRY(dev_grow(ctx, &ctx->dmc, &ctx->mc_cap, var ? xbytes + 2 * obytes : xbytes + (int64_t)sizeof(double) * maxb * call.ldo));
    call.dX = reinterpret_cast<const double*>(ctx->dmc);
    call.dout = reinterpret_cast<double*>(ctx->dmc + xbytes);
    if (var) call.dvar = reinterpret_cast<double*>(ctx->dmc + xbytes + obytes);
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dmc, X, sizeof(double) * M * d, hipMemcpyHostToDevice, ctx->stream));
    struct CallGuard {
        explicit CallGuard(PtCall* c) { g_pt = c; }
        ~CallGuard() { g_pt = nullptr; }
    } guard(&call);

    bool batched = false;
    if (B >= 2 && ctx->Np > 128 && ctx->Np <= ctx->opt_lml_batch && ctx->opt_chol == 0) {
        const BatchChain bc = {"predict_thetas", pt_chain, true, 0, 0, 2, LML_RES_INFO, lml_head};
        const bool had = ctx->have_theta;
        const int r = objective_batch_general(ctx, bc, thetas, B, 0, vlml.data(), nullptr, vinfo.data());
        if (r <= 0) note_xs_foreign(ctx, had);              // (the arena is the call's own: as a single evaluation leaves it)
        if (r < 0) { (void)hipStreamSynchronize(ctx->stream); return r; }      // nothing of this call stays in flight
        batched = r == 0;                                   // 1: no room for two scratch sets, one after another below
    }
    if (!batched) {
        call.done = 0;
        for (int64_t b = 0; b < B; b++) {
            const double* theta = thetas + b * w;
            ThetaScope at(ctx, theta);
            // Np = 128, d <= 16: gpry_lml answers from its single-launch form, which leaves no alpha_ behind -- the value
            // comes from there (its bits), the mean from the general chain at 128 padded rows
            bool fused = false;
            double fhost[2 + GPRY_THETA_MAX];
            int finf = 0;
            if (ctx->Np == 128 && ctx->opt_lml_small && ctx->opt_chol == 0) {
                StageScope s(ctx, "lml_small");
                const int r = launch_lml_small(ctx, 0, fhost, &finf);
                if (r < 0) return r;
                fused = r == 0;
            }
            double *hres, *dres;
            GPRY_TRY(objective_row(ctx, 4096, LML_RES_INFO, &hres, &dres));
            int rc, inf = 0;
            {
                StageScope s(ctx, "predict_thetas");
                rc = pt_chain(ctx, 0, dres);
            }
            at.factor_chain_ran();
            GPRY_TRY(objective_wait(ctx, "predict_thetas", rc, hres, LML_RES_INFO, &inf));
            if (fused && finf != 0) inf = finf;
            vinfo[(size_t)b] = inf;
            objective_write(ctx, inf, lml_head(fused ? fhost : hres), nullptr, nullptr, &vlml[(size_t)b], nullptr, nullptr);
        }
    }
    double ms = 0.0;
    GPRY_TRY(ns_end(ctx, &tm, &ms));
    // a theta whose matrix is not positive definite: a row of NaN, on its own
    for (int64_t b = 0; b < B; b++) {
        if (vinfo[(size_t)b] != 0)
            for (int64_t i = 0; i < M; i++) {
                mean[b * M + i] = NAN;
                if (var) var[b * M + i] = NAN;
            }
        if (lml) lml[b] = vlml[(size_t)b];
        if (info) info[b] = vinfo[(size_t)b];
    }
    if (device_ms) *device_ms = ms;
    return 0;
}

}  // namespace

extern "C" {

int gpry_predict_thetas(gpry_ctx* ctx, const double* thetas, int64_t B, const double* X, int64_t M, double* mean, double* lml,
                        int* info, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_thetas: ctx is NULL");
    return pt_run(ctx, thetas, B, X, M, mean, nullptr, lml, info, device_ms);
}

int gpry_predict_thetas_var(gpry_ctx* ctx, const double* thetas, int64_t B, const double* X, int64_t M, double* mean, double* var,
                            double* lml, int* info, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_thetas_var: ctx is NULL");
    return pt_run(ctx, thetas, B, X, M, mean, var, lml, info, device_ms);
}

}  // extern "C"
