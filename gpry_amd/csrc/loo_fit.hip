// gpry_loo_objective: the leave-one-out log predictive density of the training targets as a fit objective, with its
// theta-gradient (Rasmussen & Williams section 5.4.2; Sundararajan & Keerthi 2001).  With K^-1 = V^T V, alpha = K^-1 y_ and
// q_i = (K^-1)_ii, in transformed units like the LML:
//   L(theta) = sum_i [ 1/2 log q_i - alpha_i^2 / (2 q_i) ] - N/2 log 2 pi
//   c_i = -1/2 (1 + alpha_i^2 / q_i) / q_i  (< 0),   a = alpha / q,   b = K^-1 a,   H = diag(sqrt(-c)) K^-1
//   W'  = 1/2 (b alpha^T + alpha b^T) - H^T H
//   dL / d theta_j = sum_kl W'_kl (dK / d theta_j)_kl                 for every j at once.
// The sum over i is taken BEFORE the contraction with dK / d theta_j, so that the whole gradient is one set of traces
// against one symmetric matrix, the form lml_traces_kernel contracts with W = alpha alpha^T - K^-1.  On top of an LML
// evaluation with gradient that is one lower-only N x N x N product on the FP64 matrix pipe (the GEMM engine, A^T B),
// one matrix-vector product and gpry_loo's pass over V.
//
// One evaluation: build_factor and solve_alpha as gpry_lml's chain; loo_pass_kernel (loo.hip) and loo_fit_terms_kernel
// give q -- added ascending over the row tiles as loo_finish_kernel does, hence gpry_loo's bits --, the value's partial
// sums per 64 rows, s = sqrt(-c) and a; lauum_lower gives K^-1 (lower triangle); loo_fit_mirror_kernel writes H as a full
// square (rows scaled, lower triangle mirrored) and the per-tile partial products of b; loo_fit_bsum_kernel adds those
// ascending; the engine forms M = H^T H (lower tiles) into V's buffer; loo_fit_traces_kernel contracts W' with the
// derivative routines of kern_math.h into per-tile partial sums and loo_fit_finish_kernel adds them, and the value's, in
// a fixed order and hands everything to the host through mapped memory.  Rows and columns of the padding are masked to
// zero wherever they are read, so what the factor chain leaves there does not matter.
//
// gpry_loo_objective_batch: B thetas through ONE such chain (the arena, the chunking and the staging of gpry_lml_batch:
// objective_batch_general, api.hip).  Every kernel here takes its theta from blockIdx.z and moves its per-theta pointers by
// bset(p, blockIdx.z, bstride); C and w come from the theta's parameter row.  Tile maps, the split of the Gram product and
// every summation order are functions of the model size alone, so a theta's bits are those of a single evaluation whatever
// B, its position in the batch, the chunking and its neighbours.
//
// The evaluation works in the objective's scratch (dW, dW2, dW3, dvec, dpart, dsplit) alone: the factor held for
// prediction, a Kriging-believer session and the resident pool are not touched, and the call scratch (CallScratch, common.h)
// is not held.  L and V of the scratch are
// overwritten (H, M), so the factor cache of gpry_lml is cleared: gpry_factorize never adopts them.
#include "kern_math.h"

#define LF_T 64             // tile of the mirror pass and of the traces
#define LF_LD 65            // row stride (doubles) of the mirror pass's LDS image: row reads and column reads conflict free
#define LF_INFO 36          // host result: [value sum, grad (1 + d, + 1 with a white term) ...], status words from here

namespace {

// linear index -> (bi >= bj) of the lower block triangle, row-wise
__device__ __forceinline__ void lf_tri(int64_t t, int* bi, int* bj) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)(i + 1) * (i + 2) / 2 <= t) i++;
    while ((int64_t)i * (i + 1) / 2 > t) i--;
    *bi = i; *bj = (int)(t - (int64_t)i * (i + 1) / 2);
}

}  // namespace

// grid: Np / 64 workgroups of one wave.  q_i from the partial sums of loo_pass_kernel in loo_finish_kernel's order; the
// point's term of the value; s_i = sqrt(-c_i), a_i = alpha_i / q_i; zeros in the padding.  vpart[tile]: the tile's 64
// terms added by a fixed butterfly.
__global__ __launch_bounds__(64) void loo_fit_terms_kernel(const double* __restrict__ qpart_, int64_t Np, int64_t N, int nt,
                                                            const double* __restrict__ alpha_, double* __restrict__ q_out_,
                                                            double* __restrict__ s_out_, double* __restrict__ a_out_,
                                                            double* __restrict__ vpart_, int64_t bstride) {
    // batched launch (gpry_ctx::bn): the buffers of theta blockIdx.z
    const int z = (int)blockIdx.z;
    const double* __restrict__ qpart = bset(qpart_, z, bstride);
    const double* __restrict__ alpha = bset(alpha_, z, bstride);
    double* __restrict__ q_out = bset(q_out_, z, bstride);
    double* __restrict__ s_out = bset(s_out_, z, bstride);
    double* __restrict__ a_out = bset(a_out_, z, bstride);
    double* __restrict__ vpart = bset(vpart_, z, bstride);
    const int tb = (int)blockIdx.x, lane = threadIdx.x;
    const int64_t i = (int64_t)tb * LF_T + lane;
    double q = 0.0, s = 0.0, a = 0.0, term = 0.0;
    if (i < N) {
#pragma unroll 8
        for (int ti = tb; ti < nt; ti++) q += qpart[(int64_t)ti * Np + i];
        const double al = alpha[i], rq = 1.0 / q, u = al * al * rq;
        term = 0.5 * log(q) - 0.5 * u;
        s = sqrt(0.5 * (1.0 + u) * rq);
        a = al * rq;
    }
    q_out[i] = q; s_out[i] = s; a_out[i] = a;
    double v = term;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) vpart[tb] = v;
}

// grid: the lower-triangle 64 x 64 tiles (ti, tj) of K^-1 (lower triangle stored); 256 threads.  Writes the tile of
// H = diag(s) K^-1 and, off the diagonal, its mirror image (H is a full square), and the tile's share of b = K^-1 a:
// bpart[t][k], t = 0 .. Np / 64 - 1, holds for row k of tile row tk the product with the columns of tile t -- from tile
// (tk, t) for t <= tk, from the transpose of tile (t, tk) above it; every entry has exactly one writer.
__global__ __launch_bounds__(256) void loo_fit_mirror_kernel(const double* __restrict__ Kinv_, int64_t Np, int64_t N,
                                                             const double* __restrict__ s_, const double* __restrict__ a_,
                                                             double* __restrict__ H_, double* __restrict__ bpart_, int64_t bstride) {
    // batched launch (gpry_ctx::bn): the buffers of theta blockIdx.z -- pointer arithmetic on entry, nothing else changes
    const int z = (int)blockIdx.z;
    const double* __restrict__ Kinv = bset(Kinv_, z, bstride);
    const double* __restrict__ s = bset(s_, z, bstride);
    const double* __restrict__ a = bset(a_, z, bstride);
    double* __restrict__ H = bset(H_, z, bstride);
    double* __restrict__ bpart = bset(bpart_, z, bstride);
    __shared__ double sT[LF_T * LF_LD];
    __shared__ double sAr[LF_T], sAc[LF_T], sSr[LF_T], sSc[LF_T];
    __shared__ double sR[4 * LF_T], sC[4 * LF_T];
    int ti, tj; lf_tri(blockIdx.x, &ti, &tj);
    const bool diag = ti == tj;
    const int t = threadIdx.x, c = t & 63, rq = t >> 6;
    const int64_t row0 = (int64_t)ti * LF_T, col0 = (int64_t)tj * LF_T;
    double v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int64_t row = row0 + rq + 4 * e, col = col0 + c;
        v[e] = (row < N && col <= row) ? Kinv[row * Np + col] : 0.0;        // (col <= row < N: nothing of the padding)
    }
#pragma unroll
    for (int e = 0; e < 16; e++) sT[(rq + 4 * e) * LF_LD + c] = v[e];
    if (t < LF_T) { sAr[t] = a[row0 + t]; sSr[t] = s[row0 + t]; }
    else if (t < 2 * LF_T) { sAc[t - LF_T] = a[col0 + t - LF_T]; sSc[t - LF_T] = s[col0 + t - LF_T]; }
    __syncthreads();
    // the tile itself (a diagonal tile: both triangles), rows scaled
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int r = rq + 4 * e;
        const double x = (diag && c > r) ? sT[c * LF_LD + r] : sT[r * LF_LD + c];
        H[(row0 + r) * Np + col0 + c] = sSr[r] * x;
    }
    // its mirror image: row col0 + r of H, columns row0 + c
    if (!diag) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int r = rq + 4 * e;
            H[(col0 + r) * Np + row0 + c] = sSc[r] * sT[c * LF_LD + r];
        }
    }
    double pr = 0.0, pc = 0.0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int k = rq * 16 + e;
        const double x = (diag && k > c) ? sT[k * LF_LD + c] : sT[c * LF_LD + k];      // row c, column k
        pr = fma(x, sAc[k], pr);
        pc = fma(sT[k * LF_LD + c], sAr[k], pc);                                       // column c, row k
    }
    sR[rq * LF_T + c] = pr;
    sC[rq * LF_T + c] = pc;
    __syncthreads();
    if (t < LF_T) bpart[(int64_t)tj * Np + row0 + t] = ((sR[t] + sR[LF_T + t]) + sR[2 * LF_T + t]) + sR[3 * LF_T + t];
    else if (t < 2 * LF_T && !diag) {
        const int k = t - LF_T;
        bpart[(int64_t)ti * Np + col0 + k] = ((sC[k] + sC[LF_T + k]) + sC[2 * LF_T + k]) + sC[3 * LF_T + k];
    }
}

// b_k = sum over the tiles t ascending of bpart[t][k]
__global__ __launch_bounds__(256) void loo_fit_bsum_kernel(const double* __restrict__ bpart_, int64_t Np, int nb,
                                                           double* __restrict__ b_, int64_t bstride) {
    const double* __restrict__ bpart = bset(bpart_, (int)blockIdx.z, bstride);
    double* __restrict__ b = bset(b_, (int)blockIdx.z, bstride);
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= Np) return;
    double v = 0.0;
#pragma unroll 8
    for (int t = 0; t < nb; t++) v += bpart[(int64_t)t * Np + k];
    b[k] = v;
}

// The gradient's traces: lml_traces_kernel's tiling (kernel_build.hip: one 64 x 64 tile of pairs per workgroup, lower
// block triangle, off-diagonal tiles weighted twice, a thread owns 4 x 4 pairs, distances recomputed from the scaled
// coordinates, the coordinate loop outside the pair loops) with W'_kl = 1/2 (b_k alpha_l + alpha_k b_l) - M_kl in place of
// alpha_k alpha_l - Kinv_kl.  M holds the lower triangle.  part[tile][0 .. DP]: log C and the length scales;
// part[tile][DP + 1] (a model with a white term, diagonal tiles): sum_k (b_k alpha_k - M_kk) -- the finish multiplies by w.
template <int DP, int KID>
__global__ __launch_bounds__(256) void loo_fit_traces_kernel(
    const double* __restrict__ Xs_, const double* __restrict__ M_, int64_t ld, const double* __restrict__ alpha_,
    const double* __restrict__ b_, double* __restrict__ part_, KernParams kp, const double* __restrict__ bpar, int64_t bstride) {
    // batched launch (gpry_ctx::bn): the buffers and the constant of theta blockIdx.z, as lml_traces_kernel
    const double* __restrict__ Xs = bset(Xs_, (int)blockIdx.z, bstride);
    const double* __restrict__ M = bset(M_, (int)blockIdx.z, bstride);
    const double* __restrict__ alpha = bset(alpha_, (int)blockIdx.z, bstride);
    const double* __restrict__ b = bset(b_, (int)blockIdx.z, bstride);
    double* __restrict__ part = bset(part_, (int)blockIdx.z, bstride);
    if (bpar) kp.C = bset(bpar, (int)blockIdx.z, bstride)[0];
    // (the white entry needs no w here: the diagonal tiles leave tr W', loo_fit_finish_kernel multiplies)
    constexpr int XLD = 66;        // (lml_traces_kernel: 64 puts the sixteen k of a row into one pair of LDS banks)
    __shared__ __attribute__((aligned(16))) double Xi[DP * XLD];
    __shared__ __attribute__((aligned(16))) double Xj[DP * XLD];
    __shared__ double ai[64], aj[64], bi_[64], bj_[64];
    __shared__ double red[4][DP + 1];
    int bi, bj; lf_tri(blockIdx.x, &bi, &bj);
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    for (int e = t; e < 64 * DP; e += 256) {
        int row = e / DP, k = e - row * DP;
        double vi = 0.0, vj = 0.0;
        if (k < kp.dpad) {
            vi = Xs[((int64_t)bi * 64 + row) * kp.dpad + k];
            vj = Xs[((int64_t)bj * 64 + row) * kp.dpad + k];
        }
        Xi[k * XLD + row] = vi; Xj[k * XLD + row] = vj;
    }
    if (t < 64) { ai[t] = alpha[bi * 64 + t]; aj[t] = alpha[bj * 64 + t]; }
    else if (t < 128) { bi_[t - 64] = b[bi * 64 + t - 64]; bj_[t - 64] = b[bj * 64 + t - 64]; }
    __syncthreads();
    double g[DP + 1];
#pragma unroll
    for (int k = 0; k <= DP; k++) g[k] = 0.0;
    double r2[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) r2[a][c] = 0.0;
    int ci = ty * 4, cj = tx * 4;
    // M of the sixteen pairs, on its way while the distances are summed
    double min_[4][4];
    if (bi != bj) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const double2* pk = reinterpret_cast<const double2*>(M + ((int64_t)bi * 64 + ci + a) * ld + (int64_t)bj * 64 + cj);
            const double2 k0 = pk[0], k1 = pk[1];
            min_[a][0] = k0.x; min_[a][1] = k0.y; min_[a][2] = k1.x; min_[a][3] = k1.y;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int64_t i = (int64_t)bi * 64 + ci + a, j = (int64_t)bj * 64 + cj + c;
                min_[a][c] = M[(i > j ? i : j) * ld + (i > j ? j : i)];
            }
    }
#pragma unroll
    for (int k = 0; k < DP; k++) {
        // (two coordinates' reads in flight, the scheduler fenced behind them: see lml_traces_kernel)
        if ((k & 1) == 0) asm volatile("" : "+v"(ci), "+v"(cj));
        const double2* pi = reinterpret_cast<const double2*>(Xi + k * XLD + ci);
        const double2* pj = reinterpret_cast<const double2*>(Xj + k * XLD + cj);
        const double2 i0 = pi[0], i1 = pi[1], j0 = pj[0], j1 = pj[1];
        const double xi[4] = {i0.x, i0.y, i1.x, i1.y}, xj[4] = {j0.x, j0.y, j1.x, j1.y};
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) { const double df = xi[a] - xj[c]; r2[a][c] = fma(df, df, r2[a][c]); }
        if (k & 1) {
            asm volatile("" : "+v"(r2[0][0]), "+v"(r2[0][1]), "+v"(r2[0][2]), "+v"(r2[0][3]), "+v"(r2[1][0]), "+v"(r2[1][1]), "+v"(r2[1][2]), "+v"(r2[1][3]),
                              "+v"(r2[2][0]), "+v"(r2[2][1]), "+v"(r2[2][2]), "+v"(r2[2][3]), "+v"(r2[3][0]), "+v"(r2[3][1]), "+v"(r2[3][2]), "+v"(r2[3][3]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // r2 becomes w C h (what the second pass weighs the squared differences with)
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int il = ci + a;
        const int64_t i = (int64_t)bi * 64 + il;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int jl = cj + c;
            const int64_t j = (int64_t)bj * 64 + jl;
            double w = 0.5 * fma(bi_[il], aj[jl], ai[il] * bj_[jl]) - min_[a][c];
            double kv;
            const double h = corr_and_h<KID>(r2[a][c], &kv);
            if (i == j) kv = 1.0;
            if (i >= kp.N || j >= kp.N) w = 0.0;
            g[0] = fma(w, kp.C * kv, g[0]);
            r2[a][c] = w * kp.C * h;
        }
        __builtin_amdgcn_sched_barrier(0);      // four kernel evaluations in flight, not sixteen
    }
    asm volatile("" : "+v"(ci), "+v"(cj));
#pragma unroll
    for (int k = 0; k < DP; k++) {
        if ((k & 1) == 0) asm volatile("" : "+v"(ci), "+v"(cj));
        const double2* pi = reinterpret_cast<const double2*>(Xi + k * XLD + ci);
        const double2* pj = reinterpret_cast<const double2*>(Xj + k * XLD + cj);
        const double2 i0 = pi[0], i1 = pi[1], j0 = pj[0], j1 = pj[1];
        const double xi[4] = {i0.x, i0.y, i1.x, i1.y}, xj[4] = {j0.x, j0.y, j1.x, j1.y};
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) { const double df = xi[a] - xj[c]; g[1 + k] = fma(r2[a][c], df * df, g[1 + k]); }
        if (k & 1) {
            asm volatile("" : "+v"(g[k]), "+v"(g[1 + k]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int k = 0; k <= DP; k++) {
        double v = g[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (t <= DP) {
        double sum = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        if (bi != bj) sum *= 2.0;
        part[(int64_t)blockIdx.x * (DP + 2) + t] = sum;
    }
    // d K / d log w = w I: tr W' = sum_k (b_k alpha_k - M_kk), formed by the diagonal tiles; 0 off the diagonal
    if (kp.white_on && wave == 1) {
        double v = 0.0;
        if (bi == bj) {
            const int64_t i = (int64_t)bi * 64 + lane;
            if (i < kp.N) v = bi_[lane] * ai[lane] - M[i * ld + i];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) part[(int64_t)blockIdx.x * (DP + 2) + DP + 1] = v;
    }
}

// Last kernel of an evaluation.  Workgroup k < nth (with a gradient): entry k of the gradient, strided partial sums and
// a fixed LDS tree as reduce_traces_kernel; workgroup 0 also adds the value's partial sums ascending and hands the
// factorisation status on.  Everything goes straight into the mapped host buffer: theta blockIdx.z of a batched launch
// writes row blockIdx.z (GPRY_BRES_STRIDE doubles) and multiplies the white entry by ITS w (parameter row).
static_assert(LF_INFO + 3 <= GPRY_BRES_STRIDE, "result row too short");
__global__ __launch_bounds__(256) void loo_fit_finish_kernel(const double* __restrict__ part_, int64_t ntile, int stride, int want_grad,
                                                             int nplain, int white_col, double white,
                                                             const double* __restrict__ vpart_, int nv, const int* __restrict__ info_,
                                                             double* __restrict__ host_res, const double* __restrict__ bpar,
                                                             int64_t bstride) {
    const int tb = (int)blockIdx.z;
    if (bpar) white = bset(bpar, tb, bstride)[GPRY_BPAR_WHITE];
    const double* __restrict__ part = bset(part_, tb, bstride);
    const double* __restrict__ vpart = bset(vpart_, tb, bstride);
    const int* __restrict__ info = bset(info_, tb, bstride);
    host_res += (int64_t)tb * GPRY_BRES_STRIDE;
    __shared__ double red[256];
    const int k = blockIdx.x, t = threadIdx.x;
    if (want_grad) {
        const int col = k < nplain ? k : white_col;
        double s = 0.0;
        for (int64_t i = t; i < ntile; i += 256) s += part[i * stride + col];
        red[t] = s;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w) red[t] += red[t + w];
            __syncthreads();
        }
        if (t == 0) host_res[1 + k] = k >= nplain ? red[0] * white : red[0];
    }
    if (k == 0 && t == 0) {
        double v = 0.0;
        for (int i = 0; i < nv; i++) v += vpart[i];
        host_res[0] = v;
        host_res[LF_INFO] = (double)info[0]; host_res[LF_INFO + 1] = (double)info[1];
        host_res[LF_INFO + 2] = (double)info[3];        // (0x5A..: a bounded wait of the panel step ran out)
    }
}

namespace {

// What an evaluation needs of the partial-sum buffer and of the split-K scratch -- functions of the model size alone.  The
// single evaluation grows the context's buffers to it before its first launch; a batched one sizes the arena's pieces by it.
// part: q and w of the pass over V | b | traces -- and solve_alpha's partial sums, which are done with by then.
struct LooFitPlan {
    int nt, nb, DPsel, nsplit;                      // row tiles with training rows, 64-row tiles, width class of the traces, split of M = H^T H
    int64_t ntile, o_q, o_w, o_b, o_tr, need;       // offsets into the partial sums and their total (doubles)
};
LooFitPlan loo_fit_plan(const gpry_ctx* ctx) {
    LooFitPlan p;
    const int64_t Np = ctx->Np;
    p.nt = (int)((ctx->N + LF_T - 1) / LF_T); p.nb = (int)(Np / LF_T);
    p.ntile = (int64_t)p.nb * (p.nb + 1) / 2;
    p.DPsel = dp_class(ctx->d);
    p.o_q = 0; p.o_w = p.o_q + (int64_t)p.nt * Np; p.o_b = p.o_w + (int64_t)p.nt * Np; p.o_tr = p.o_b + (int64_t)p.nb * Np;
    p.need = p.o_tr + p.ntile * (p.DPsel + 2);
    const int64_t need_solve = ((Np + 255) / 256) * Np;
    if (p.need < need_solve) p.need = need_solve;
    // the split of K^-1 = V^T V's engine launch (lauum_lower)
    p.nsplit = splitk_count((Np / 128) * (Np / 128 + 1) / 2, Np);
    return p;
}

// the launches of one evaluation at the theta the context holds -- or, in a batched evaluation (gpry_ctx::bn), at the bn
// thetas whose parameter rows sit in the arena; results and status land in `dres` (mapped host memory; theta tb at row tb
// of GPRY_BRES_STRIDE doubles)
int loo_fit_chain(gpry_ctx* ctx, int want_grad, double* dres) {
    const int64_t Np = ctx->Np, N = ctx->N;
    const LooFitPlan pl = loo_fit_plan(ctx);
    const int nt = pl.nt, nb = pl.nb, DPsel = pl.DPsel;
    const int64_t ntile = pl.ntile, o_q = pl.o_q, o_w = pl.o_w, o_b = pl.o_b, o_tr = pl.o_tr;
    // Sized before the first launch: nothing is re-allocated under way.  (A batched evaluation works in the arena: its
    // pieces were sized by the same plan and never grow.)
    if (pl.need > ctx->part_cap && ctx->bpar) return gpry_fail(ctx, -1, "batched chain: partial sums exceed the arena");
    GPRY_TRY(dev_grow(ctx, &ctx->dpart, &ctx->part_cap, pl.need));
    const unsigned bn = (unsigned)ctx->bn;
    const int64_t bs = ctx->bstride;
    GPRY_TRY(build_factor(ctx, ctx->dW, ctx->dW2, ctx->dW3, nullptr));
    hipStream_t st = ctx->stream;
    double* dz = ctx->dvec;                 // z = V y
    double* da = ctx->dvec + Np;            // alpha
    double* dq = ctx->dvec + 3 * Np;        // q, s = sqrt(-c), a = alpha / q, b = K^-1 a, the value's partial sums
    double *ds = dq + Np, *daq = ds + Np, *db = daq + Np, *dvp = db + Np;
    double* part = ctx->dpart;
    {
        StageScope s(ctx, "solve_alpha");
        GPRY_TRY(solve_alpha(ctx, ctx->dW2, ctx->dy, dz, da, Np));
    }
    {
        StageScope s(ctx, "loo_q");
        GPRY_TRY(loo_pass_launch(ctx, ctx->dW2, part + o_q, part + o_w));
        hipLaunchKernelGGL(loo_fit_terms_kernel, dim3((unsigned)nb, 1, bn), dim3(LF_T), 0, st, part + o_q, Np, N, nt, da, dq, ds, daq,
                           dvp, bs);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (want_grad) {
        {
            StageScope s(ctx, "lauum");
            GPRY_TRY(lauum_lower(ctx, ctx->dW2, ctx->dW3, Np));
        }
        {
            // H into dW: L is dead (the objective needs no log-determinant)
            StageScope s(ctx, "loo_mirror");
            hipLaunchKernelGGL(loo_fit_mirror_kernel, dim3((unsigned)ntile, 1, bn), dim3(256), 0, st, ctx->dW3, Np, N, ds, daq, ctx->dW,
                               part + o_b, bs);
            hipLaunchKernelGGL(loo_fit_bsum_kernel, dim3((unsigned)((Np + 255) / 256), 1, bn), dim3(256), 0, st, part + o_b, Np, nb, db, bs);
            HIP_TRY(ctx, hipGetLastError());
        }
        {
            // M = H^T H, lower tiles, into V's buffer (V is dead behind lauum); the split of K^-1 = V^T V's engine launch
            StageScope s(ctx, "loo_gram");
            GemmArgs g = {};
            g.A = ctx->dW; g.lda = Np; g.B = ctx->dW; g.ldb = Np; g.C = ctx->dW2; g.ldc = Np;
            g.M = (int)Np; g.N = (int)Np; g.K = (int)Np;
            g.kmode = KM_FULL; g.lower_only = 1; g.tile_map = TM_ROWMAJOR; g.info = ctx->dinfo;
            const int nsplit = pl.nsplit;
            if (nsplit > 1) {
                double* sbuf = nullptr;
                GPRY_TRY(gemm_split_scratch(ctx, nsplit, Np * Np, &sbuf));
                g.nsplit = nsplit; g.split_buf = sbuf; g.split_stride = Np * Np;
            }
            g.small64 = 1;          // Np is a multiple of 128
            GPRY_TRY(gemm_f64_launch(ctx, g, true, false, EPI_STORE));
        }
    }
    StageScope s(ctx, "loo_traces");
    const KernParams kp = make_kp(ctx);
    if (want_grad) {
#define LFT2(DP, KID) hipLaunchKernelGGL((loo_fit_traces_kernel<DP, KID>), dim3((unsigned)ntile, 1, bn), dim3(256), 0, st, ctx->dXs, \
                                         ctx->dW2, Np, da, db, part + o_tr, kp, ctx->bpar, bs)
#define LFT4(KID) { if (DPsel == 4) LFT2(4, KID); else if (DPsel == 8) LFT2(8, KID); \
                    else if (DPsel == 16) LFT2(16, KID); else if (DPsel == 24) LFT2(24, KID); else LFT2(32, KID); }
        DISPATCH_KID(ctx->kernel_id, LFT4)
#undef LFT4
#undef LFT2
        HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(loo_fit_finish_kernel, dim3((unsigned)(want_grad ? ctx_ntheta(ctx) : 1), 1, bn), dim3(256), 0, st, part + o_tr,
                       ntile, DPsel + 2, want_grad, ctx->d + 1, DPsel + 1, kp.white, dvp, nb, ctx->dinfo, dres, ctx->bpar, bs);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int gpry_loo_objective(gpry_ctx* ctx, const double* theta, int want_grad, double* value, double* grad, int* info) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_loo_objective: ctx is NULL");
    if (!theta || !value || (want_grad && !grad))
        return gpry_fail(ctx, -1, "loo_objective: theta, value and (with want_grad) grad must not be NULL");
    GPRY_TRY(objective_entry(ctx, "loo_objective", theta, 1));
    double *hres, *dres;
    GPRY_TRY(objective_row(ctx, 4096, LF_INFO, &hres, &dres));
    int inf = 0;
    {
        ThetaScope at(ctx, theta);      // L and V of the scratch are overwritten: by the factor, then by H and M
        const int rc = loo_fit_chain(ctx, want_grad, dres);
        at.factor_chain_ran();
        GPRY_TRY(objective_wait(ctx, "loo_objective", rc, hres, LF_INFO, &inf));
    }
    if (info) *info = inf;
    objective_write(ctx, inf, hres[0], hres + 1, nullptr, value, want_grad ? grad : nullptr, nullptr);
    return 0;
}

// B evaluations in one call: the optimiser runs of a "loo" fit stepped side by side (gpry_amd/lockstep.py), as gpry_lml_batch
// serves the LML's (the reference runs its restarts one after another, gpry/gpr.py:968-984).  From Np = 128 -- there is no
// single-launch form of this objective -- up to option "lml_batch": ONE chain of launches for all thetas of a chunk
// (objective_batch_general, api.hip, with loo_fit_chain as its chain), always in the latency schedule: option "lml_schedule"
// concerns gpry_lml_batch alone.  Above that, with the rocSOLVER comparator or where fewer than two scratch sets fit: one
// gpry_loo_objective after another.  Either way every theta gets the launches of a single evaluation, hence its bits.
int gpry_loo_objective_batch(gpry_ctx* ctx, const double* thetas, int64_t B, int want_grad, double* value, double* grad, int* info) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_loo_objective_batch: ctx is NULL");
    if (B <= 0) return gpry_fail(ctx, -1, "loo_objective_batch: B = %lld thetas", (long long)B);
    if (!thetas || !value || (want_grad && !grad))
        return gpry_fail(ctx, -1, "loo_objective_batch: thetas, value and (with want_grad) grad must not be NULL");
    GPRY_TRY(objective_entry(ctx, "loo_objective_batch", thetas, B));
    const int w = ctx_ntheta(ctx);
    if (B >= 2 && ctx->Np >= 128 && ctx->Np <= ctx->opt_lml_batch && ctx->opt_chol == 0) {
        const LooFitPlan pl = loo_fit_plan(ctx);
        const BatchChain bc = {"loo_batch", loo_fit_chain, true, pl.need, pl.nsplit > 1 ? (int64_t)pl.nsplit * ctx->Np * ctx->Np : 0,
                               1, LF_INFO, [](const double* o) { return o[0]; }};
        const bool had = ctx->have_theta;
        const int r = objective_batch_general(ctx, bc, thetas, B, want_grad, value, grad, info);
        if (r <= 0) {
            note_xs_foreign(ctx, had);                                  // (the arena is the call's own: as the single call leaves it)
            if (r < 0) (void)hipStreamSynchronize(ctx->stream);         // nothing of this call stays in flight
            return r;
        }                               // 1: no room for two scratch sets, one after another below
    }
    for (int64_t b = 0; b < B; b++) {
        int inf = 0;
        GPRY_TRY(gpry_loo_objective(ctx, thetas + b * w, want_grad, value + b, want_grad ? grad + b * w : nullptr, &inf));
        if (info) info[b] = inf;
    }
    return 0;
}

}  // extern "C"
