// Cross-validation of the training set from the resident factor: the kernels behind gpry_loo (leave-one-out and
// one-step-ahead) and gpry_leave_out (leave-group-out).  Rasmussen & Williams section 5.4.2: with V = L^-1, K^-1 = V^T V
// and alpha_ = K^-1 y_, all at the current theta and with the pre-processors as they are,
//   leave-one-out     q_i = (K^-1)_ii = sum_k V_ki^2:   y_i | rest  ~  N(y_i - alpha_i / q_i, 1 / q_i);
//   leave-group-out   B = (K^-1)_GG = V[:, G]^T V[:, G]: y_G | rest  ~  N(y_G - B^-1 alpha_G, B^-1);
//   one-step-ahead    w = V y_:   y_k | y_0 .. y_k-1  ~  N(y_k - w_k / V_kk, 1 / V_kk^2), z-score w_k.
// What the host makes of them (z-scores, coverage, log densities) is gpry_amd/mc.py: validate_gp.
//
// gpry_loo is one pass over the lower triangle of V in 64 x 64 tiles (loo_pass_kernel: the tile goes through LDS, read
// with the lanes along the columns; a tile gives 64 partial column sums of squares and 64 partial row products with y_)
// and loo_finish_kernel, which adds a column's partials over the row tiles and a row's over the column tiles, both
// ascending, and forms the outputs in units of y.  The tiling is a function of the model size alone and both sums are
// always formed, so q_i and w_k are the same bits on any context and whatever the call asks for.
//
// gpry_leave_out: the host sorts every group's indices (the outputs are handed back in the caller's order), so that a
// group's results do not depend on the order of its indices.  lgo_gram_kernel: one workgroup per (group, chunk of 256
// training rows) gathers the group's columns of V 32 rows at a time into LDS -- zeros in the columns that pad the group
// to a multiple of 16 -- and accumulates the lower 16 x 16 tiles of V_G^T V_G with v_mfma_f64_16x16x4_f64; chunks that
// end above the group's smallest index hold zeros only (V is lower triangular) and are skipped.  lgo_finish_kernel: one
// workgroup per group adds the chunks ascending, puts the identity on the padding's diagonal, factors B in LDS (the
// 16 x 16 pieces of chol16.h, one wave), inverts the factor column by column into the unused upper triangle, and forms
// delta = B^-1 alpha_G, B^-1 = W^T W, chi^2 and log det.  A group is one fixed chain of operations on its own columns:
// the same bits whatever other groups share the call and wherever it stands in the list.  gpry_predict_without
// (predict_without.hip) runs the same two kernels through lgo.h and takes W and z = W alpha_G from the finish.
//
// Both read V, alpha_, y_ and the noise vector and write to the call scratch alone (CallScratch, common.h), which each holds
// for the length of the call: the state of predict, of the sweep, of a Kriging-believer session and of the samplers is not
// touched.
#include "ns_common.h"
#include "chol16.h"
#include "lgo.h"
#include <algorithm>
#include <vector>

#define LOO_T 64            // tile of the pass over V
#define LOO_LD 65           // row stride (doubles) of its LDS image: column reads and row reads both conflict free

// grid: the lower-triangle tiles (ti, tj), tj <= ti, of the leading nt x nt tiles; 256 threads.  grid.z: the thetas of a
// batched objective (gpry_ctx::bn) -- V and the partial sums of theta blockIdx.z lie bstride doubles further on; y is shared
__global__ __launch_bounds__(256) void loo_pass_kernel(const double* __restrict__ V_, int64_t Np, int64_t N,
                                                       const double* __restrict__ y, double* __restrict__ qpart_,
                                                       double* __restrict__ wpart_, int64_t bstride) {
    const double* __restrict__ V = bset(V_, (int)blockIdx.z, bstride);
    double* __restrict__ qpart = bset(qpart_, (int)blockIdx.z, bstride);
    double* __restrict__ wpart = bset(wpart_, (int)blockIdx.z, bstride);
    __shared__ double sV[LOO_T * LOO_LD];
    __shared__ double sY[LOO_T];
    __shared__ double sQ[4 * LOO_T], sW[4 * LOO_T];
    const int tl = blockIdx.x;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tl) ti++;
    const int tj = tl - ti * (ti + 1) / 2;
    const int t = threadIdx.x, c = t & 63, rq = t >> 6;
    const int64_t row0 = (int64_t)ti * LOO_T, col0 = (int64_t)tj * LOO_T, col = col0 + c;
    double v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int64_t row = row0 + rq + 4 * e;
        v[e] = (row < N && col <= row) ? V[row * Np + col] : 0.0;      // (col <= row < N: nothing of the padding)
    }
#pragma unroll
    for (int e = 0; e < 16; e++) sV[(rq + 4 * e) * LOO_LD + c] = v[e];
    if (t < LOO_T) sY[t] = col < N ? y[col] : 0.0;
    __syncthreads();
    double sq = 0.0, sw = 0.0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const double a = sV[(rq * 16 + e) * LOO_LD + c];               // column c, rows 16 rq ..
        sq = fma(a, a, sq);
        sw = fma(sV[c * LOO_LD + rq * 16 + e], sY[rq * 16 + e], sw);   // row c, columns 16 rq ..
    }
    sQ[rq * LOO_T + c] = sq;
    sW[rq * LOO_T + c] = sw;
    __syncthreads();
    if (t < LOO_T) qpart[(int64_t)ti * Np + col0 + t] = ((sQ[t] + sQ[LOO_T + t]) + sQ[2 * LOO_T + t]) + sQ[3 * LOO_T + t];
    else if (t < 2 * LOO_T) {
        const int r = t - LOO_T;
        wpart[(int64_t)tj * Np + row0 + r] = ((sW[r] + sW[LOO_T + r]) + sW[2 * LOO_T + r]) + sW[3 * LOO_T + r];
    }
}

// out: five rows of N doubles: mean, var_y, var_f, seq_mean, seq_var_y
__global__ __launch_bounds__(64) void loo_finish_kernel(const double* __restrict__ V, int64_t Np, int64_t N, int nt,
                                                         const double* __restrict__ qpart, const double* __restrict__ wpart,
                                                         const double* __restrict__ y, const double* __restrict__ alpha_,
                                                         const double* __restrict__ noise, double white, int white_on, double y_mean, double y_std,
                                                         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * LOO_T + threadIdx.x;      // one wave per tile of 64 points: N / 64 workgroups
    if (i >= N) return;
    const int tb = (int)blockIdx.x;
    double q = 0.0, w = 0.0;
#pragma unroll 8
    for (int ti = tb; ti < nt; ti++) q += qpart[(int64_t)ti * Np + i];
#pragma unroll 8
    for (int tj = 0; tj <= tb; tj++) w += wpart[(int64_t)tj * Np + i];
    const double vkk = V[i * (Np + 1)], ys2 = y_std * y_std, yi = y[i], rq = 1.0 / q;
    out[i] = ns_rn((yi - alpha_[i] * rq) * y_std) + y_mean;
    out[N + i] = ys2 * rq;
    out[2 * N + i] = fmax(rq - (white_on ? noise[i] + white : noise[i]), 0.0) * ys2;      // var_f: without alpha_i + w
    out[3 * N + i] = ns_rn((yi - w / vkk) * y_std) + y_mean;
    out[4 * N + i] = ys2 / (vkk * vkk);
}

// tile number -> (ta, tb), tb <= ta, row-wise
__device__ __forceinline__ void lgo_tile(int tl, int* ta, int* tb) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= tl) a++;
    *ta = a; *tb = tl - a * (a + 1) / 2;
}

// grid: (groups of the batch, chunks of LGO_KC rows); 256 threads = 4 waves, wave w owns the tiles w, w + 4, w + 8
__global__ __launch_bounds__(256) void lgo_gram_kernel(const double* __restrict__ V, int64_t Np, int64_t N,
                                                       const int* __restrict__ idx, const LgoGroup* __restrict__ groups,
                                                       double* __restrict__ part) {
    __shared__ double sP[LGO_KS * LGO_LD];
    const LgoGroup G = groups[blockIdx.x];
    const int chunk = blockIdx.y;
    if (chunk < G.c0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = t & 63, rq = t >> 6;
    const int nb = G.np / 16, ntile = nb * (nb + 1) / 2;
    const int64_t my = c < G.n ? (int64_t)idx[G.idx_off + c] : -1;
    const int64_t k0 = (int64_t)chunk * LGO_KC, kend = k0 + LGO_KC < N ? k0 + LGO_KC : N;
    v4d acc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int64_t ks = k0; ks < kend; ks += LGO_KS) {
        double v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t row = ks + rq + 4 * e;
            v[e] = (my >= 0 && row < kend && my <= row) ? V[row * Np + my] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) sP[(rq + 4 * e) * LGO_LD + c] = v[e];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int tl = wave + 4 * q;
            if (tl < ntile) {
                int ta, tb;
                lgo_tile(tl, &ta, &tb);
                acc[q] = c16::mfma_tn<LGO_LD>(acc[q], sP + 16 * ta, sP + 16 * tb, LGO_KS, lane);
            }
        }
        __syncthreads();
    }
    double* dst = part + G.part_off + (int64_t)(chunk - G.c0) * G.np * G.np;
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int tl = wave + 4 * q;
        if (tl < ntile) {
            int ta, tb;
            lgo_tile(tl, &ta, &tb);
#pragma unroll
            for (int u = 0; u < 4; u++) dst[(16 * ta + g + 4 * u) * G.np + 16 * tb + r] = acc[q][u];
        }
    }
}

// grid: the groups of the batch; 256 threads.  W = L^-1 lives in the upper triangle of sB as its transpose (W_ka at
// sB[a][k], k > a) with its diagonal in swd.
__global__ __launch_bounds__(256) void lgo_finish_kernel(const double* __restrict__ part, const LgoGroup* __restrict__ groups,
                                                         const int* __restrict__ idx, const double* __restrict__ alpha_,
                                                         const double* __restrict__ y, int nch, double y_mean, double y_std,
                                                         double* __restrict__ omean, double* __restrict__ ocov,
                                                         double* __restrict__ ochi2, double* __restrict__ ologpdf,
                                                         int* __restrict__ oinfo, double* __restrict__ oW, double* __restrict__ oz) {
    __shared__ double sB[LGO_MAX * LGO_LD];
    __shared__ double sa[LGO_MAX], sz[LGO_MAX], sdl[LGO_MAX], srd[LGO_MAX], swd[LGO_MAX];
    __shared__ int sbad;
    const LgoGroup G = groups[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = G.n, np = G.np, nb = np / 16, nc = nch - G.c0;
    const double* src = part + G.part_off;
    for (int e = t; e < np * np; e += 256) {
        const int a = e / np, b = e - a * np;
        double s = 0.0;
        if (b <= a) {
            if (a < n) for (int c = 0; c < nc; c++) s += src[(int64_t)c * np * np + e];
            else s = a == b ? 1.0 : 0.0;
        }
        sB[a * LGO_LD + b] = s;
    }
    if (t < LGO_MAX) sa[t] = t < n ? alpha_[idx[G.idx_off + t]] : 0.0;
    __syncthreads();
    if (wave == 0) {                       // right-looking Cholesky by 16 x 16 blocks
        int bad = 0;
        for (int j = 0; j < nb; j++) {
            double* Ljj = sB + (16 * j) * LGO_LD + 16 * j;
            const int bj = c16::chol16_wave<LGO_LD>(Ljj, srd + 16 * j, lane);
            if (bj && !bad) bad = 16 * j + bj;
            c16::wave_fence();
            for (int i = j + 1; i < nb; i++) c16::trsm16_rows<LGO_LD>(sB + (16 * i) * LGO_LD + 16 * j, Ljj, srd + 16 * j, lane);
            c16::wave_fence();
            for (int i = j + 1; i < nb; i++)
                for (int c = j + 1; c <= i; c++) {
                    double* T = sB + (16 * i) * LGO_LD + 16 * c;
                    v4d acc = c16::tile_load<LGO_LD>(T, lane);
                    acc = c16::mfma_nt<LGO_LD, true>(acc, sB + (16 * i) * LGO_LD + 16 * j, sB + (16 * c) * LGO_LD + 16 * j, 16, lane);
                    c16::tile_store<LGO_LD>(T, acc, lane);
                }
            c16::wave_fence();
        }
        if (lane == 0) sbad = bad;
    }
    __syncthreads();
    const int bad = sbad;
    if (bad) {                             // not positive definite: this group alone reports it
        for (int e = t; ocov && e < n * n; e += 256) ocov[G.cov_off + e] = NAN;
        if (omean && t < n) omean[G.idx_off + t] = NAN;
        if (oW) {
            for (int e = t; e < LGO_MAX * LGO_MAX; e += 256) oW[(int64_t)blockIdx.x * LGO_MAX * LGO_MAX + e] = 0.0;
            if (t < LGO_MAX) oz[(int64_t)blockIdx.x * LGO_MAX + t] = 0.0;
        }
        if (t == 0) { ochi2[blockIdx.x] = NAN; ologpdf[blockIdx.x] = NAN; oinfo[blockIdx.x] = bad; }
        return;
    }
    if (t < np) {                          // column t of W by forward substitution
        const double wd = 1.0 / sB[t * LGO_LD + t];
        swd[t] = wd;
        for (int i = t + 1; i < np; i++) {
            double s = -sB[i * LGO_LD + t] * wd;
            for (int j = t + 1; j < i; j++) s = fma(-sB[i * LGO_LD + j], sB[t * LGO_LD + j], s);
            sB[t * LGO_LD + i] = s / sB[i * LGO_LD + i];
        }
    }
    __syncthreads();
    if (t < np) {                          // z = W alpha_G
        double s = 0.0;
        for (int j = 0; j < t; j++) s = fma(sB[j * LGO_LD + t], sa[j], s);
        sz[t] = fma(swd[t], sa[t], s);
    }
    __syncthreads();
    if (t < np) {                          // delta = W^T z
        double s = swd[t] * sz[t];
        for (int k = t + 1; k < np; k++) s = fma(sB[t * LGO_LD + k], sz[k], s);
        sdl[t] = s;
    }
    __syncthreads();
    if (omean && t < n) omean[G.idx_off + t] = ns_rn((y[idx[G.idx_off + t]] - sdl[t]) * y_std) + y_mean;
    // gpry_predict_without (predict_without.hip): W dense, row k = [W_k0 .. W_kk, 0 ...], and z = W alpha_G, zeros in the padding
    if (oW) {
        double* Wg = oW + (int64_t)blockIdx.x * LGO_MAX * LGO_MAX;
        const int a = t & 63;
        for (int k = t >> 6; k < LGO_MAX; k += 4) {
            double w = 0.0;
            if (k < n && a < k) w = sB[a * LGO_LD + k];
            if (k < n && a == k) w = swd[k];
            Wg[k * LGO_MAX + a] = w;
        }
        if (t < LGO_MAX) oz[(int64_t)blockIdx.x * LGO_MAX + t] = t < n ? sz[t] : 0.0;
    }
    if (t == 0) {
        double chi = 0.0, ld = 0.0;
        for (int i = 0; i < n; i++) { chi = fma(sa[i], sdl[i], chi); ld += log(sB[i * LGO_LD + i]); }
        ochi2[blockIdx.x] = chi;
        ologpdf[blockIdx.x] = -0.5 * chi + ld - (double)n * (0.9189385332046727 + log(y_std));
        oinfo[blockIdx.x] = 0;
    }
    const double ys2 = y_std * y_std;
    for (int e = t; ocov && e < n * n; e += 256) { // (B^-1)_ab = sum over k >= max(a, b) of W_ka W_kb: the same chain for (a, b) and (b, a)
        const int a = e / n, b = e - a * n, hi = a > b ? a : b, lo = a > b ? b : a;
        double s = (hi == lo ? swd[hi] : sB[lo * LGO_LD + hi]) * swd[hi];
        for (int k = hi + 1; k < n; k++) s = fma(sB[a * LGO_LD + k], sB[b * LGO_LD + k], s);
        ocov[G.cov_off + e] = s * ys2;
    }
}

namespace {

int loo_require(gpry_ctx* ctx, const char* who) {
    if (ctx->N <= 0 || !ctx->have_theta || !ctx->factor_valid)
        return gpry_fail(ctx, -1, "%s: the context holds no valid factor (call gpry_factorize)", who);
    return 0;
}

}  // namespace

// the checks of a list of groups and the groups in ascending index order, for gpry_leave_out and gpry_predict_without
// (predict_without.hip); perm: place in the caller's group of the sorted group's entries; *ncov: the sum of n^2
int lgo_parse_groups(gpry_ctx* ctx, const char* who, const int64_t* idx, const int64_t* offsets, int64_t ngroups,
                     std::vector<LgoGroup>* groups_, std::vector<int>* sidx_, std::vector<int>* perm_, int64_t* ncov) {
    if (!idx || !offsets) return gpry_fail(ctx, -1, "%s: idx or offsets is NULL", who);
    if (ngroups < 1 || ngroups > LGO_MAX_GROUPS)
        return gpry_fail(ctx, -1, "%s: ngroups = %lld, need 1 <= ngroups <= %d", who, (long long)ngroups, LGO_MAX_GROUPS);
    const int64_t N = ctx->N;
    std::vector<LgoGroup>& groups = *groups_;
    std::vector<int>&sidx = *sidx_, &perm = *perm_;
    groups.assign((size_t)ngroups, LgoGroup());
    sidx.clear(); perm.clear();
    if (offsets[0] != 0) return gpry_fail(ctx, -1, "%s: offsets[0] = %lld, need 0", who, (long long)offsets[0]);
    std::vector<std::pair<int64_t, int>> srt;
    int64_t cov_off = 0;
    for (int64_t g = 0; g < ngroups; g++) {
        const int64_t n = offsets[g + 1] - offsets[g];
        if (n < 1) return gpry_fail(ctx, -1, "%s: group %lld is empty", who, (long long)g);
        if (n > LGO_MAX) return gpry_fail(ctx, -1, "%s: group %lld has %lld points, at most %d", who, (long long)g, (long long)n, LGO_MAX);
        srt.clear();
        for (int64_t a = 0; a < n; a++) {
            const int64_t i = idx[offsets[g] + a];
            if (i < 0 || i >= N)
                return gpry_fail(ctx, -1, "%s: index %lld of group %lld is outside [0, %lld)", who, (long long)i, (long long)g, (long long)N);
            srt.push_back({i, (int)a});
        }
        std::sort(srt.begin(), srt.end());
        for (int64_t a = 1; a < n; a++)
            if (srt[(size_t)a].first == srt[(size_t)a - 1].first)
                return gpry_fail(ctx, -1, "%s: group %lld holds index %lld more than once", who, (long long)g, (long long)srt[(size_t)a].first);
        LgoGroup& G = groups[(size_t)g];
        G.idx_off = (int64_t)sidx.size(); G.cov_off = cov_off; G.part_off = 0;
        G.n = (int)n; G.np = (int)round_up(n, 16); G.c0 = (int)(srt[0].first / LGO_KC); G.pad = 0;
        cov_off += n * n;
        for (int64_t a = 0; a < n; a++) { sidx.push_back((int)srt[(size_t)a].first); perm.push_back(srt[(size_t)a].second); }
    }
    *ncov = cov_off;
    return 0;
}

// the Gram and the finish of `ng` groups whose partial Grams fit `dpart` (LgoGroup::part_off), on the context's factor.  oW, oz
// (nullable, gpry_predict_without): W = L_B^-1, 64 x 64 dense per group, and z = W alpha_G, 64 per group; omean, ocov nullable
void lgo_launch(gpry_ctx* ctx, const int* didx, const LgoGroup* dgroups, int64_t ng, double* dpart, double* omean, double* ocov,
                double* ochi2, double* ologpdf, int* oinfo, double* oW, double* oz) {
    const int nch = (int)((ctx->N + LGO_KC - 1) / LGO_KC);
    hipLaunchKernelGGL(lgo_gram_kernel, dim3((unsigned)ng, (unsigned)nch), dim3(256), 0, ctx->stream, ctx->dV, ctx->Np, ctx->N, didx,
                       dgroups, dpart);
    hipLaunchKernelGGL(lgo_finish_kernel, dim3((unsigned)ng), dim3(256), 0, ctx->stream, dpart, dgroups, didx, ctx->dalpha_, ctx->dy,
                       nch, ctx->tf.y_mean, ctx->tf.y_std, omean, ocov, ochi2, ologpdf, oinfo, oW, oz);
}

// the pass of gpry_loo over another inverse factor (loo_fit.hip: the V of an objective evaluation): the same launch, so
// the partial sums -- and q_i once they are added ascending -- are the bits gpry_loo forms for the same model
int loo_pass_launch(gpry_ctx* ctx, const double* V, double* qpart, double* wpart) {
    const int nt = (int)((ctx->N + LOO_T - 1) / LOO_T);
    hipLaunchKernelGGL(loo_pass_kernel, dim3((unsigned)(nt * (nt + 1) / 2), 1, (unsigned)ctx->bn), dim3(256), 0, ctx->stream, V, ctx->Np,
                       ctx->N, ctx->dy, qpart, wpart, ctx->bstride);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" {

int gpry_loo(gpry_ctx* ctx, double* mean, double* var_y, double* var_f, double* seq_mean, double* seq_var_y,
             double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_loo: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(loo_require(ctx, "gpry_loo"));
    const int64_t N = ctx->N, Np = ctx->Np;
    const int nt = (int)((N + LOO_T - 1) / LOO_T);
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    // the call scratch: the two rows of partial sums of the pass over V, the five output rows.  The two kernels below are
    // all this call launches, on ctx->stream, which ns_end drains.
    CallScratch cs(ctx, "gpry_loo");
    const auto rq = cs.take<double>((int64_t)nt * Np), rw = cs.take<double>((int64_t)nt * Np), rout = cs.take<double>(5 * N);
    GPRY_TRY(cs.claim());
    const int64_t out_bytes = 8 * 5 * N;
    if (out_bytes > ctx->hloo_cap) {
        if (ctx->hloo) HIP_TRY(ctx, hipHostFree(ctx->hloo));
        ctx->hloo = nullptr; ctx->hloo_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->hloo, (size_t)out_bytes, hipHostMallocDefault));
        ctx->hloo_cap = out_bytes;
    }
    double *qpart = cs.at(rq), *wpart = cs.at(rw), *out = cs.at(rout);
    hipStream_t st = ctx->stream;
    {
        StageScope scope(ctx, "loo");
        hipLaunchKernelGGL(loo_pass_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, ctx->dV, Np, N, ctx->dy,
                           qpart, wpart, (int64_t)0);
        hipLaunchKernelGGL(loo_finish_kernel, dim3((unsigned)nt), dim3(LOO_T), 0, st, ctx->dV, Np, N, nt, qpart, wpart, ctx->dy,
                           ctx->dalpha_, ctx->dnoise, ctx_white(ctx), ctx->white ? 1 : 0, ctx->tf.y_mean, ctx->tf.y_std, out);
        HIP_TRY(ctx, hipGetLastError());
        // one copy of the five rows into pinned memory of the call's own, handed out below
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hloo, out, out_bytes, hipMemcpyDeviceToHost, st));
    }
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    double* dst[5] = {mean, var_y, var_f, seq_mean, seq_var_y};
    for (int k = 0; k < 5; k++)
        if (dst[k]) memcpy(dst[k], (const double*)ctx->hloo + k * N, sizeof(double) * N);
    return 0;
}

int gpry_leave_out(gpry_ctx* ctx, const int64_t* idx, const int64_t* offsets, int64_t ngroups, double* mean, double* cov,
                   double* chi2, double* logpdf, int* info, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_leave_out: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(loo_require(ctx, "gpry_leave_out"));
    const int64_t N = ctx->N;
    const int nch = (int)((N + LGO_KC - 1) / LGO_KC);
    std::vector<LgoGroup> groups;
    std::vector<int> sidx, perm;
    int64_t cov_off = 0;
    GPRY_TRY(lgo_parse_groups(ctx, "gpry_leave_out", idx, offsets, ngroups, &groups, &sidx, &perm, &cov_off));
    const int64_t ncov = cov_off, nidx = (int64_t)sidx.size();
    // batches of groups whose partial Grams fit LGO_BATCH_DOUBLES (a group's bits do not depend on its batch)
    int64_t part_max = 0;
    std::vector<int64_t> batch_first(1, 0);
    {
        int64_t cur = 0;
        for (int64_t g = 0; g < ngroups; g++) {
            LgoGroup& G = groups[(size_t)g];
            const int64_t need = (int64_t)(nch - G.c0) * G.np * G.np;
            if (cur > 0 && cur + need > LGO_BATCH_DOUBLES) { batch_first.push_back(g); cur = 0; }
            G.part_off = cur;
            cur += need;
            part_max = std::max(part_max, cur);
        }
        batch_first.push_back(ngroups);
    }
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    // the call scratch, in this order.  lgo_launch takes every buffer from its caller, and all of the call is queued on
    // ctx->stream, which ns_end drains.
    CallScratch cs(ctx, "gpry_leave_out");
    const auto rgroups = cs.take<LgoGroup>(ngroups); const auto ridx = cs.take<int>(nidx);
    const auto rmean = cs.take<double>(nidx), rcov = cs.take<double>(ncov), rchi = cs.take<double>(ngroups), rlp = cs.take<double>(ngroups);
    const auto rinfo = cs.take<int>(ngroups); const auto rpart = cs.take<double>(part_max);
    GPRY_TRY(cs.claim());
    LgoGroup* dgroups = cs.at(rgroups);
    int *didx = cs.at(ridx), *dinfo = cs.at(rinfo);
    double *dmean = cs.at(rmean), *dcov = cs.at(rcov), *dchi = cs.at(rchi), *dlp = cs.at(rlp), *dpart = cs.at(rpart);
    std::vector<double> hmean((size_t)nidx), hcov((size_t)ncov);
    hipStream_t st = ctx->stream;
    {
        StageScope scope(ctx, "leave_out");
        HIP_TRY(ctx, hipMemcpyAsync(dgroups, groups.data(), sizeof(LgoGroup) * ngroups, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(didx, sidx.data(), sizeof(int) * nidx, hipMemcpyHostToDevice, st));
        for (size_t bi = 0; bi + 1 < batch_first.size(); bi++) {
            const int64_t g0 = batch_first[bi], ng = batch_first[bi + 1] - g0;
            lgo_launch(ctx, didx, dgroups + g0, ng, dpart, dmean, dcov, dchi + g0, dlp + g0, dinfo + g0, nullptr, nullptr);
        }
        HIP_TRY(ctx, hipGetLastError());
        if (mean) HIP_TRY(ctx, hipMemcpyAsync(hmean.data(), dmean, sizeof(double) * nidx, hipMemcpyDeviceToHost, st));
        if (cov) HIP_TRY(ctx, hipMemcpyAsync(hcov.data(), dcov, sizeof(double) * ncov, hipMemcpyDeviceToHost, st));
        if (chi2) HIP_TRY(ctx, hipMemcpyAsync(chi2, dchi, sizeof(double) * ngroups, hipMemcpyDeviceToHost, st));
        if (logpdf) HIP_TRY(ctx, hipMemcpyAsync(logpdf, dlp, sizeof(double) * ngroups, hipMemcpyDeviceToHost, st));
        if (info) HIP_TRY(ctx, hipMemcpyAsync(info, dinfo, sizeof(int) * ngroups, hipMemcpyDeviceToHost, st));
    }
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    // back to the caller's order inside every group
    for (int64_t g = 0; g < ngroups; g++) {
        const LgoGroup& G = groups[(size_t)g];
        const int* p = perm.data() + G.idx_off;
        const int64_t o = offsets[g];
        for (int a = 0; mean && a < G.n; a++) mean[o + p[a]] = hmean[(size_t)(G.idx_off + a)];
        for (int a = 0; cov && a < G.n; a++)
            for (int c = 0; c < G.n; c++)
                cov[G.cov_off + (int64_t)p[a] * G.n + p[c]] = hcov[(size_t)(G.cov_off + (int64_t)a * G.n + c)];
    }
    return 0;
}

}  // extern "C"
