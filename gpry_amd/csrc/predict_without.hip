// gpry_predict_without: what the surrogate would predict at arbitrary points if a group G of training points had never
// been bought -- at the same theta, y map, noise vector and white term, from the factor the context holds, without a
// refactorisation.  With V = L^-1, alpha_ = K^-1 y_ and B = (K^-1)_GG = L_B L_B^T, W = L_B^-1 (what gpry_leave_out forms):
//   t = W alpha_G                 (n entries),
//   S = W (V_G^T V)               (n x N: W times the group's rows of K^-1),
//   s(x) = S k*(x),   mean_-G(x) - mean(x) = -y_std s.t,   var_-G(x) - var(x) = +y_std^2 |s|^2
// (the block-inverse downdate of K^-1; the prior variance cancels, so nothing is clamped).  The means are the unclipped,
// ungated ones, the variances the latent ones.
//
// Setup, per batch of groups (PW_ROWS stacked padded rows at the most, a group padded to a multiple of 16 by zero rows):
//   lgo_gram_kernel, lgo_finish_kernel   loo.hip's own kernels through lgo_launch (lgo.h): B, its factor, W and t carry the
//                           bits gpry_leave_out works with;
//   pw_gather_kernel        VG[k, r] = V[k, G_r] for k >= G_r, zeros elsewhere and in the padding, k-major;
//   gemm_f64_launch         P = VG^T V on the FP64 MFMA engine (TN, KM_B_LOWER: k from the column tile's first row on -- the
//                           rows of V above it hold zeros only), split over k into pw_nsplit(Np) slices added in order;
//   pw_apply_kernel         S = W P, 16 stacked rows per workgroup row, b ascending; the columns from N on are zeros.
// Points, per panel of PW_PC points:
//   pv_panel_launch         the cross-kernel panel of gpry_predict_thetas_var (predict_thetas.hip: pt_var_panel_kernel), the
//                           same point scaling and correlation routine, at the context's own theta;
//   gemm_f64_launch         s = S K* (NN, dense k, the same split), the stacked rows of all groups of the batch at once;
//   pw_finish_kernel        per (group, point): sum of s^2 and of s t over the group's rows, ascending.
// Every element of an MFMA product is an accumulation chain of its own, in k order; all shapes handed to the engine are
// multiples of 128, so the engine's variant does not depend on the call; the split is a function of Np alone.  Hence
// dmean[g, i] and dvar[g, i] depend on the model, the group as a set and the point alone: not on M, positions, the split
// of points or groups over calls, panels or batches, the other groups of the call or the context.  A point whose k*
// underflows gives s = 0 exactly, and 0 and 0.
//
// State: reads V, alpha_, y_ and the scaled training rows; writes the call scratch (CallScratch, common.h), which it holds
// for the length of the call, and the staging buffer ctx->dmc (the points of one upload).  The scratch, in doubles, with
// R = min(PW_ROWS, the largest batch's rows rounded up to 128),
// pc = min(PW_PC, M rounded up to 128) and ns = pw_nsplit(Np):
//   3 R Np  (VG, P, S)  +  Np pc  (panel)  +  R pc  (s)  +  ns R max(Np, pc)  (slices, ns > 1)  +  2 (R / 16) pc  (outputs)
//   + the partial Grams of a batch (gpry_leave_out's, at most LGO_BATCH_DOUBLES) + 4160 per group of a batch (W, t)
// and a few integers per group.
#include "ns_common.h"
#include "lgo.h"
#include <algorithm>

#define PW_ROWS 1024        // stacked padded rows of one batch of groups: 64 groups of up to 16 points, 16 of 64
#define PW_PC 2048          // points per panel
#define PW_XC 32768         // points per upload into the staging buffer (a multiple of PW_PC)

// slices of k in both products: a function of the model size alone
static inline int pw_nsplit(int64_t Np) { return Np >= 4096 ? 8 : Np >= 2048 ? 4 : Np >= 1024 ? 2 : 1; }

// grid (Np, R / 128), 128 threads
__global__ __launch_bounds__(128) void pw_gather_kernel(const double* __restrict__ V, int64_t Np, int64_t N,
                                                        const int* __restrict__ rowidx, int R, double* __restrict__ VG) {
    const int64_t k = blockIdx.x;
    const int r = (int)blockIdx.y * 128 + threadIdx.x;
    if (r >= R) return;
    const int i = rowidx[r];
    VG[k * R + r] = (i >= 0 && k < N && (int64_t)i <= k) ? V[k * Np + i] : 0.0;
}

// grid (Np / 256 rounded up, R / 16), 256 threads: 16 stacked rows x 256 columns.  rbmap[rb] = (group within the batch,
// 16-row block within the group), or (-1, 0) behind the last group
__global__ __launch_bounds__(256) void pw_apply_kernel(const double* __restrict__ P, int64_t Np, int64_t N, const int2* __restrict__ rbmap,
                                                       const double* __restrict__ W, double* __restrict__ S) {
    __shared__ double sW[16 * LGO_MAX];
    const int rb = blockIdx.y, t = threadIdx.x;
    const int2 m = rbmap[rb];
    const int64_t j = (int64_t)blockIdx.x * 256 + t;
    if (m.x < 0) {
        if (j < Np)
            for (int a = 0; a < 16; a++) S[((int64_t)16 * rb + a) * Np + j] = 0.0;
        return;
    }
    for (int e = t; e < 16 * LGO_MAX; e += 256) sW[e] = W[(int64_t)m.x * LGO_MAX * LGO_MAX + (int64_t)16 * m.y * LGO_MAX + e];
    __syncthreads();
    if (j >= Np) return;
    double s[16];
#pragma unroll
    for (int a = 0; a < 16; a++) s[a] = 0.0;
    const int64_t r0 = (int64_t)16 * (rb - m.y);
    for (int bb = 0; bb <= m.y; bb++) {        // (W is lower triangular: its entries right of the diagonal are exact zeros)
        double p[16];
#pragma unroll
        for (int b = 0; b < 16; b++) p[b] = P[(r0 + 16 * bb + b) * Np + j];
#pragma unroll
        for (int a = 0; a < 16; a++)
#pragma unroll
            for (int b = 0; b < 16; b++) s[a] = fma(sW[a * LGO_MAX + 16 * bb + b], p[b], s[a]);
    }
#pragma unroll
    for (int a = 0; a < 16; a++) S[((int64_t)16 * rb + a) * Np + j] = j < N ? s[a] : 0.0;
}

// grid (points / 256 rounded up, groups of the batch), 256 threads
__global__ __launch_bounds__(256) void pw_finish_kernel(const double* __restrict__ sv, int64_t lds, const int* __restrict__ grow0,
                                                        const int* __restrict__ gn, const double* __restrict__ z, int64_t npts,
                                                        double y_std, double ys2, double* __restrict__ omean, double* __restrict__ ovar,
                                                        int64_t ldo) {
    const int g = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= npts) return;
    const int64_t r0 = grow0[g];
    const int n = gn[g];
    double ss = 0.0, st = 0.0;
    for (int a = 0; a < n; a++) {
        const double v = sv[(r0 + a) * lds + c];
        ss = fma(v, v, ss);
        st = fma(v, z[(int64_t)g * LGO_MAX + a], st);
    }
    omean[(int64_t)g * ldo + c] = 0.0 - y_std * st;
    ovar[(int64_t)g * ldo + c] = ys2 * ss;
}

extern "C" {

int gpry_predict_without(gpry_ctx* ctx, const int64_t* idx, const int64_t* offsets, int64_t ngroups, const double* X, int64_t M,
                         double* dmean, double* dvar, int* info, double* device_ms) {
    const char* who = "gpry_predict_without";
    if (!ctx) return gpry_fail(nullptr, -1, "%s: ctx is NULL", who);
    GPRY_TRY(serve_stop(ctx));
    if (!idx || !offsets || !X) return gpry_fail(ctx, -1, "%s: idx, offsets or X is NULL", who);
    if (!dmean && !dvar) return gpry_fail(ctx, -1, "%s: dmean and dvar are both NULL", who);
    if (ngroups < 1 || M < 1) return gpry_fail(ctx, -1, "%s: ngroups = %lld, M = %lld", who, (long long)ngroups, (long long)M);
    if (ctx->N <= 0 || !ctx->have_theta || !ctx->factor_valid)
        return gpry_fail(ctx, -1, "%s: the context holds no valid factor (call gpry_factorize)", who);
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "%s: d = %d > %d", who, ctx->d, GPRY_MAX_DIM);
    const int d = ctx->d;
    const int64_t N = ctx->N, Np = ctx->Np;
    GPRY_TRY(check_points_finite(ctx, who, X, M));
    GPRY_TRY(check_x_affine(ctx, who));
    std::vector<LgoGroup> groups;
    std::vector<int> sidx, perm;
    int64_t ncov = 0;
    GPRY_TRY(lgo_parse_groups(ctx, who, idx, offsets, ngroups, &groups, &sidx, &perm, &ncov));
    const int64_t nidx = (int64_t)sidx.size();
    const int nch = (int)((N + LGO_KC - 1) / LGO_KC);

    // batches of groups: at most PW_ROWS stacked rows and LGO_BATCH_DOUBLES of partial Grams (a group's bits depend on neither)
    std::vector<int64_t> batch_first(1, 0);
    std::vector<int> grow0((size_t)ngroups), gn((size_t)ngroups);
    int64_t part_max = 0, rows_max = 0, gb_max = 0;
    {
        int64_t cur = 0, rows = 0;
        for (int64_t g = 0; g < ngroups; g++) {
            LgoGroup& G = groups[(size_t)g];
            const int64_t need = (int64_t)(nch - G.c0) * G.np * G.np;
            if (rows > 0 && (rows + G.np > PW_ROWS || cur + need > LGO_BATCH_DOUBLES)) { batch_first.push_back(g); cur = 0; rows = 0; }
            G.part_off = cur;
            grow0[(size_t)g] = (int)rows; gn[(size_t)g] = G.n;
            cur += need; rows += G.np;
            part_max = std::max(part_max, cur);
            rows_max = std::max(rows_max, rows);
            gb_max = std::max(gb_max, g + 1 - batch_first.back());
        }
        batch_first.push_back(ngroups);
    }
    const int64_t nbatch = (int64_t)batch_first.size() - 1;
    const int64_t R = round_up(rows_max, 128), pcw = std::min<int64_t>(PW_PC, round_up(M, 128));
    const int ns = pw_nsplit(Np);
    // the stacked rows of every batch: the training index of a row (-1: padding) and the map of its 16-row blocks
    std::vector<int> rowidx((size_t)(nbatch * R), -1);
    std::vector<int2> rbmap((size_t)(nbatch * (R / 16)), make_int2(-1, 0));
    for (int64_t b = 0; b < nbatch; b++)
        for (int64_t g = batch_first[(size_t)b]; g < batch_first[(size_t)b + 1]; g++) {
            const LgoGroup& G = groups[(size_t)g];
            for (int a = 0; a < G.n; a++) rowidx[(size_t)(b * R + grow0[(size_t)g] + a)] = sidx[(size_t)(G.idx_off + a)];
            for (int q = 0; q < G.np / 16; q++)
                rbmap[(size_t)(b * (R / 16) + grow0[(size_t)g] / 16 + q)] = make_int2((int)(g - batch_first[(size_t)b]), q);
        }

    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    GPRY_TRY(ensure_pred_xs(ctx));
    // The call scratch, in this order.  lgo_launch and pv_panel_launch take their buffers from here, the GEMM engine its
    // slices (`split`), so nothing below claims it again; the points of an upload go through the staging buffer dmc, which is
    // no part of it.  Everything is queued on ctx->stream, which ns_end drains.
    CallScratch cs(ctx, who);
    const auto rgroups = cs.take<LgoGroup>(ngroups); const auto ridx = cs.take<int>(nidx), rinfo = cs.take<int>(ngroups);
    const auto rchilp = cs.take<double>(2 * ngroups), rW = cs.take<double>(LGO_MAX * LGO_MAX * gb_max), rz = cs.take<double>(LGO_MAX * gb_max);
    const auto rrowidx = cs.take<int>(nbatch * R); const auto rrbmap = cs.take<int2>(nbatch * (R / 16));
    const auto rgrow0gn = cs.take<int>(2 * ngroups);
    const auto rpart = cs.take<double>(part_max), rVG = cs.take<double>(Np * R), rP = cs.take<double>(R * Np), rS = cs.take<double>(R * Np),
               rKst = cs.take<double>(Np * pcw), rsv = cs.take<double>(R * pcw),
               rsplit = cs.take<double>(ns > 1 ? ns * R * std::max(Np, pcw) : 0), rom = cs.take<double>(gb_max * pcw),
               rov = cs.take<double>(gb_max * pcw);
    GPRY_TRY(cs.claim());
    const int64_t xc = std::min<int64_t>(PW_XC, M);
    GPRY_TRY(dev_grow(ctx, &ctx->dmc, &ctx->mc_cap, (int64_t)sizeof(double) * xc * d));
    LgoGroup* dgroups = cs.at(rgroups);
    int *didx = cs.at(ridx), *dinfo = cs.at(rinfo), *drowidx = cs.at(rrowidx), *dgrow0 = cs.at(rgrow0gn), *dgn = dgrow0 + ngroups;
    int2* drbmap = cs.at(rrbmap);
    double *dchi = cs.at(rchilp), *dlp = dchi + ngroups, *dW = cs.at(rW), *dz = cs.at(rz), *dpart = cs.at(rpart), *VG = cs.at(rVG),
           *P = cs.at(rP), *S = cs.at(rS), *Kst = cs.at(rKst), *sv = cs.at(rsv), *split = cs.at(rsplit), *om = cs.at(rom), *ov = cs.at(rov);
    double* dX = reinterpret_cast<double*>(ctx->dmc);
    hipStream_t st = ctx->stream;
    const double y_std = ctx->tf.y_std, ys2 = y_std * y_std;
    std::vector<int> hinfo((size_t)ngroups, 0);
    HIP_TRY(ctx, hipMemcpyAsync(dgroups, groups.data(), sizeof(LgoGroup) * ngroups, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(didx, sidx.data(), sizeof(int) * nidx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(drowidx, rowidx.data(), sizeof(int) * nbatch * R, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(drbmap, rbmap.data(), sizeof(int2) * nbatch * (R / 16), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dgrow0, grow0.data(), 4 * ngroups, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dgn, gn.data(), 4 * ngroups, hipMemcpyHostToDevice, st));
    for (int64_t b = 0; b < nbatch; b++) {
        const int64_t g0 = batch_first[(size_t)b], ng = batch_first[(size_t)b + 1] - g0;
        {
            StageScope scope(ctx, "without_setup");
            lgo_launch(ctx, didx, dgroups + g0, ng, dpart, nullptr, nullptr, dchi + g0, dlp + g0, dinfo + g0, dW, dz);
            hipLaunchKernelGGL(pw_gather_kernel, dim3((unsigned)Np, (unsigned)(R / 128)), dim3(128), 0, st, ctx->dV, Np, N,
                               drowidx + b * R, (int)R, VG);
            HIP_TRY(ctx, hipGetLastError());
            GemmArgs g = {};
            g.A = VG; g.lda = R; g.B = ctx->dV; g.ldb = Np; g.C = P; g.ldc = Np;
            g.M = (int)R; g.N = (int)Np; g.K = (int)Np;
            g.kmode = KM_B_LOWER; g.tile_map = TM_ROWMAJOR;
            if (ns > 1) { g.nsplit = ns; g.split_buf = split; g.split_stride = R * Np; }
            GPRY_TRY(gemm_f64_launch(ctx, g, true, false, EPI_STORE));
            hipLaunchKernelGGL(pw_apply_kernel, dim3((unsigned)((Np + 255) / 256), (unsigned)(R / 16)), dim3(256), 0, st, P, Np, N,
                               drbmap + b * (R / 16), dW, S);
            HIP_TRY(ctx, hipGetLastError());
        }
        for (int64_t x0 = 0; x0 < M; x0 += PW_XC) {
            const int64_t nx = std::min<int64_t>(PW_XC, M - x0);
            HIP_TRY(ctx, hipMemcpyAsync(dX, X + x0 * d, sizeof(double) * nx * d, hipMemcpyHostToDevice, st));
            for (int64_t p0 = 0; p0 < nx; p0 += PW_PC) {
                const int64_t np = std::min<int64_t>(PW_PC, nx - p0), cols = round_up(np, 128);
                StageScope scope(ctx, "without_points");
                {
                    StageScope sp(ctx, "without_panel");
                    GPRY_TRY(pv_panel_launch(ctx, dX + p0 * d, np, cols, Kst, pcw));
                }
                {
                    StageScope sc(ctx, "without_contract");
                    GemmArgs g = {};
                    g.A = S; g.lda = Np; g.B = Kst; g.ldb = pcw; g.C = sv; g.ldc = pcw;
                    g.M = (int)R; g.N = (int)cols; g.K = (int)Np;
                    g.kmode = KM_FULL; g.tile_map = TM_ROWMAJOR;
                    if (ns > 1) { g.nsplit = ns; g.split_buf = split; g.split_stride = R * pcw; }
                    GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
                }
                hipLaunchKernelGGL(pw_finish_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)ng), dim3(256), 0, st, sv, pcw,
                                   dgrow0 + g0, dgn + g0, dz, np, y_std, ys2, om, ov, pcw);
                HIP_TRY(ctx, hipGetLastError());
                if (dmean)
                    HIP_TRY(ctx, hipMemcpy2DAsync(dmean + g0 * M + x0 + p0, sizeof(double) * M, om, sizeof(double) * pcw,
                                                  sizeof(double) * np, (size_t)ng, hipMemcpyDeviceToHost, st));
                if (dvar)
                    HIP_TRY(ctx, hipMemcpy2DAsync(dvar + g0 * M + x0 + p0, sizeof(double) * M, ov, sizeof(double) * pcw,
                                                  sizeof(double) * np, (size_t)ng, hipMemcpyDeviceToHost, st));
            }
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(hinfo.data(), dinfo, sizeof(int) * ngroups, hipMemcpyDeviceToHost, st));
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    // a group whose block of K^-1 is not positive definite: its rows are NaN, on their own
    for (int64_t g = 0; g < ngroups; g++) {
        if (hinfo[(size_t)g] != 0)
            for (int64_t i = 0; i < M; i++) {
                if (dmean) dmean[g * M + i] = NAN;
                if (dvar) dvar[g * M + i] = NAN;
            }
        if (info) info[g] = hinfo[(size_t)g];
    }
    return 0;
}

}  // extern "C"
