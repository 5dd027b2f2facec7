// gpry_lml_hessian: the Hessian of the log marginal likelihood in theta = [log C, log l_1 .. log l_d (, log w)], in closed
// form (Rasmussen & Williams eq. 5.9 differentiated once more).  With K = C k(r^2) + diag(alpha + w), alpha_ = K^-1 y_,
// W = alpha_ alpha_^T - K^-1, K_i = dK / dtheta_i, K_ij = d2K / dtheta_i dtheta_j:
//   H_ij = 1/2 tr(W K_ij) - (K_i alpha_)^T K^-1 (K_j alpha_) + 1/2 tr(K^-1 K_i K^-1 K_j)
//   K_0 = C k (no noise), K_i = C h D_i, K_w = w I;  K_00 = K_0, K_0i = K_i, K_ww = w I, every other entry with log w is 0;
//   K_ij = C (g D_i D_j - 2 delta_ij h D_i) for two length scales, g = -2 dh / dr^2, defined as 0 at r = 0 (D_i D_j = 0 there).
//
// One evaluation (lml_hess_chain), every stage one launch or one engine call:
//   (a) gpry_lml's chain with gradient: build_factor, solve_alpha, log det, lauum_lower (K^-1, lower), the gradient traces --
//       the same launches on the same operands, hence gpry_lml's bits for value and gradient;
//   (b) lml_hess_mirror_kernel writes K^-1 as a full square (zeros in the padding); lml_hess_pairs_kernel, one 64 x 64 tile
//       of pairs per workgroup over the full square, computes r^2, h and g once per pair, writes the d matrices K_i as full
//       zero-padded squares, the tile's share of the products K_i alpha_ and -- with v_mfma_f64_16x16x4 -- the tile's weighted
//       Gram sum_ab (W_ab C g_ab) D_i D_j (d <= 16: one 16 x 16 accumulator; above: low-low, high-low, high-high);
//   (c) B_i = K^-1 K_i for the d length scales: ONE batched launch of the GEMM engine (the explicit-inverse route, see
//       profiles/lml_hessian.md);
//   (d) lml_hess_btraces_kernel: 1/2 tr(B_i B_j) for all i, j as a Gram over the tile pairs (a, b) / (b, a) on the matrix pipe,
//       every B read once per tile pair; B_0 = I - K^-1 diag(alpha + w) and B_w = w K^-1 are formed from K^-1 on the fly;
//   (e) u_i = V (K_i alpha_) for all p columns (K_0 alpha_ = y_ - (alpha + w) alpha_, K_w alpha_ = w alpha_), middle = u_i . u_j;
//   (f) lml_hess_finish_kernel: one workgroup per entry i <= j adds the per-tile partial sums by a strided pass and a fixed
//       LDS tree, assembles H and writes it and its mirror image into mapped host memory.
// Tile maps and summation orders are functions of (N, d, kernel) alone.  The evaluation works in the objective's scratch
// (dW, dW2, dW3, dvec, dpart, dsplit) and in the call scratch (CallScratch, common.h), which it holds until it has waited
// for the chain: the factor held for prediction, a Kriging-believer session and the resident pool are not touched; the
// factor cache of gpry_lml is cleared.
#include "kern_math.h"

#define LH_T 64
#define LH_LD 65            // row stride of the mirror pass's LDS image
#define LH_XLD 66           // row stride of the coordinate images (lml_traces_kernel)
#define LH_INFO LML_RES_INFO             // host result: gpry_lml's row [logdet/2, quad, grad ...], status words from here
#define LH_HOFF 1024                     // ... and H, p x p row-major, from here (behind the units of the single-launch objective)
#define LH_MAX_NP 4096

namespace {

// linear index -> (bi >= bj) of the lower block triangle, row-wise
__device__ __forceinline__ void lh_tri(int64_t t, int* bi, int* bj) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)(i + 1) * (i + 2) / 2 <= t) i++;
    while ((int64_t)i * (i + 1) / 2 > t) i--;
    *bi = i; *bj = (int)(t - (int64_t)i * (i + 1) / 2);
}

// k, h (d k / d log l_i = h D_i) and g = -2 dh / dr^2 of a pair, all without the factor C; g = 0 at r = 0
template <int KID>
__device__ __forceinline__ void corr_h_g(double r2, double* kv, double* h, double* g) {
    if (KID == GPRY_RBF) {
        const double e = fast_exp_neg(0.5 * r2);
        *kv = e; *h = e; *g = r2 != 0.0 ? e : 0.0;
        return;
    }
    if (KID == GPRY_MATERN12) {
        const double r = fast_sqrt_pos(r2), e = fast_exp_neg(r);
        *kv = e;
        if (r != 0.0) { *h = e / r; *g = e * (1.0 + r) / (r * r * r); }
        else { *h = 0.0; *g = 0.0; }
        return;
    }
    if (KID == GPRY_MATERN32) {
        const double t = fast_sqrt_pos(r2) * SQRT3, e = fast_exp_neg(t);
        *kv = (1.0 + t) * e; *h = 3.0 * e; *g = t != 0.0 ? 9.0 * e / t : 0.0;
        return;
    }
    const double t = fast_sqrt_pos(r2) * SQRT5, e = fast_exp_neg(t);
    *kv = (1.0 + t + t * t * (1.0 / 3.0)) * e;
    *h = (5.0 / 3.0) * (t + 1.0) * e;
    *g = r2 != 0.0 ? (25.0 / 3.0) * e : 0.0;
}

// sum of v over the 256 threads: the fixed LDS tree of reduce_traces_kernel (valid in every thread)
__device__ __forceinline__ double lh_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

}  // namespace

// grid: the lower-triangle 64 x 64 tiles (ti, tj) of K^-1 (lower triangle stored); 256 threads.  Writes the tile and, off
// the diagonal, its mirror image into the full square Kf; rows and columns of the padding become zeros.
__global__ __launch_bounds__(256) void lml_hess_mirror_kernel(const double* __restrict__ Kinv, int64_t Np, int64_t N,
                                                              double* __restrict__ Kf) {
    __shared__ double sT[LH_T * LH_LD];
    int ti, tj; lh_tri(blockIdx.x, &ti, &tj);
    const bool diag = ti == tj;
    const int t = threadIdx.x, c = t & 63, rq = t >> 6;
    const int64_t row0 = (int64_t)ti * LH_T, col0 = (int64_t)tj * LH_T;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int64_t row = row0 + rq + 4 * e, col = col0 + c;
        sT[(rq + 4 * e) * LH_LD + c] = (row < N && col <= row) ? Kinv[row * Np + col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int r = rq + 4 * e;
        Kf[(row0 + r) * Np + col0 + c] = (diag && c > r) ? sT[c * LH_LD + r] : sT[r * LH_LD + c];
    }
    if (!diag) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int r = rq + 4 * e;
            Kf[(col0 + r) * Np + row0 + c] = sT[c * LH_LD + r];
        }
    }
}

// grid: nb * nb tiles (bi, bj) of the full square of pairs; 256 threads.  Wave w, lane (g = lane >> 4, r = lane & 15) owns
// the sixteen pairs (row 16 g + e, column 16 w + r), e = 0 .. 15, in the first phase: r^2, h, g once per pair, the entries
// of K_k = C h D_k for every length scale (rows of 128 contiguous bytes) and the tile's share of K_k alpha_ -- by the
// symmetry of K_k the column sums over the tile's rows: mvpart[bi][k][column], exactly one writer per entry.  Second phase:
// the Gram of the pairs' D vectors weighted by W C g on the matrix pipe; a wave contracts the pairs it owns, four at a time
// (lane group g: pair (16 g + e, 16 w + cc)), lane (g, r) supplies coordinate r (and 16 + r) of its group's pair, the weight
// comes from the lane that owns the pair.  The four waves are combined as (w0 + w1) + (w2 + w3).
// gpart[tile][block][256]: block 0 = low-low, and for d > 16 block 1 = high-low, block 2 = high-high; 16 x 16 row-major.
// KM_ONLY (gpry_var_theta_grad's setup, lml_hess_km_launch below): the first phase's matrices K_k alone -- Kf, alpha, gpart
// and mvpart are not touched.
template <int NBK, int KID, bool KM_ONLY = false>
__global__ __launch_bounds__(256) void lml_hess_pairs_kernel(const double* __restrict__ Xs, const double* __restrict__ Kf, int64_t Np,
                                                             const double* __restrict__ alpha, double* __restrict__ Km,
                                                             double* __restrict__ gpart, double* __restrict__ mvpart, KernParams kp,
                                                             int nb) {
    constexpr int XR = NBK * 16, NB2 = NBK == 1 ? 1 : 3;      // NBK: blocks of 16 coordinates (1: d <= 16, 2: d <= 32)
    __shared__ double Xi[XR * LH_XLD];
    __shared__ double Xj[XR * LH_XLD];
    __shared__ double ai[64], aj[64];
    __shared__ double gred[4 * NB2 * 256];
    const int bi = (int)blockIdx.x / nb, bj = (int)blockIdx.x - bi * nb;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, g = lane >> 4, r = lane & 15;
    for (int e = t; e < 64 * XR; e += 256) {
        const int row = e / XR, k = e - row * XR;
        double vi = 0.0, vj = 0.0;
        if (k < kp.d) {
            vi = Xs[((int64_t)bi * 64 + row) * kp.dpad + k];
            vj = Xs[((int64_t)bj * 64 + row) * kp.dpad + k];
        }
        Xi[k * LH_XLD + row] = vi; Xj[k * LH_XLD + row] = vj;
    }
    if (!KM_ONLY) {
        if (t < 64) ai[t] = alpha[bi * 64 + t];
        else if (t < 128) aj[t - 64] = alpha[bj * 64 + t - 64];
    }
    __syncthreads();
    const int col = 16 * w + r;
    const int64_t gcol = (int64_t)bj * 64 + col, grow0 = (int64_t)bi * 64 + 16 * g;
    double ch[16], wg[16];
#pragma unroll
    for (int e = 0; e < 16; e++) ch[e] = 0.0;          // r^2 first
    for (int k = 0; k < kp.d; k++) {
        const double xj = Xj[k * LH_XLD + col];
#pragma unroll
        for (int e = 0; e < 16; e++) { const double df = Xi[k * LH_XLD + 16 * g + e] - xj; ch[e] = fma(df, df, ch[e]); }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) {
        double kv, h, gg;
        corr_h_g<KID>(ch[e], &kv, &h, &gg);
        const bool in = grow0 + e < kp.N && gcol < kp.N;
        ch[e] = in ? kp.C * h : 0.0;
        if (KM_ONLY) continue;
        const double kf = Kf[(grow0 + e) * Np + gcol];
        const double W = ai[16 * g + e] * aj[col] - kf;
        wg[e] = in ? W * (kp.C * gg) : 0.0;
    }
    const int64_t sq = Np * Np;
    for (int k = 0; k < kp.d; k++) {
        const double xj = Xj[k * LH_XLD + col];
        double mv = 0.0;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const double df = Xi[k * LH_XLD + 16 * g + e] - xj;
            const double v = ch[e] * (df * df);
            Km[(int64_t)k * sq + (grow0 + e) * Np + gcol] = v;
            if (!KM_ONLY) mv = fma(v, ai[16 * g + e], mv);
        }
        if (KM_ONLY) continue;
        mv += __shfl_xor(mv, 16);
        mv += __shfl_xor(mv, 32);
        if (g == 0) mvpart[((int64_t)bi * kp.d + k) * Np + gcol] = mv;
    }
    if (KM_ONLY) return;
    // the weighted Gram on the matrix pipe (operand and accumulator layout: chol16.h)
    v4d acc[NB2];
#pragma unroll
    for (int b = 0; b < NB2; b++) acc[b] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const double xi0 = Xi[r * LH_XLD + 16 * g + e];
        const double xi1 = NBK == 2 ? Xi[(16 + r) * LH_XLD + 16 * g + e] : 0.0;
#pragma unroll 4
        for (int cc = 0; cc < 16; cc++) {
            const double wgt = __shfl(wg[e], (lane & 48) | cc);
            const int c2 = 16 * w + cc;
            const double d0 = xi0 - Xj[r * LH_XLD + c2], D0 = d0 * d0;
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wgt * D0, D0, acc[0], 0, 0, 0);
            if (NBK == 2) {
                const double d1 = xi1 - Xj[(16 + r) * LH_XLD + c2], D1 = d1 * d1;
                acc[NB2 - 2] = __builtin_amdgcn_mfma_f64_16x16x4f64(wgt * D1, D0, acc[NB2 - 2], 0, 0, 0);
                acc[NB2 - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(wgt * D1, D1, acc[NB2 - 1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB2; b++)
#pragma unroll
        for (int q = 0; q < 4; q++) gred[(w * NB2 + b) * 256 + (g + 4 * q) * 16 + r] = acc[b][q];
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB2; b++)
        gpart[((int64_t)blockIdx.x * NB2 + b) * 256 + t] =
            (gred[b * 256 + t] + gred[(NB2 + b) * 256 + t]) + (gred[(2 * NB2 + b) * 256 + t] + gred[(3 * NB2 + b) * 256 + t]);
}

// the right-hand sides K_i alpha_, column i of theta at R[i * Np ..]: log C: y_ - (alpha + w) alpha_; a length scale: the
// tiles' shares added ascending over the row tiles; log w: w alpha_.  Zeros in the padding.  grid ((Np + 255) / 256, p).
__global__ __launch_bounds__(256) void lml_hess_rhs_kernel(const double* __restrict__ mvpart, const double* __restrict__ y,
                                                           const double* __restrict__ noise, const double* __restrict__ alpha,
                                                           int64_t Np, int64_t N, int d, int nb, double white, double* __restrict__ R) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)blockIdx.y;
    if (m >= Np) return;
    double v = 0.0;
    if (m < N) {
        if (i == 0) v = y[m] - (noise[m] + white) * alpha[m];
        else if (i <= d) {
#pragma unroll 8
            for (int tb = 0; tb < nb; tb++) v += mvpart[((int64_t)tb * d + (i - 1)) * Np + m];
        } else v = white * alpha[m];
    }
    R[(int64_t)i * Np + m] = v;
}

// u_i = V R_i (V lower triangular; only its entries with column <= row < N are read).  grid (Np / 64, p); a wave owns 16
// rows, the lanes walk a row's columns 64 at a time, the 64 partial sums are added by a fixed butterfly.
__global__ __launch_bounds__(256) void lml_hess_trmv_kernel(const double* __restrict__ V, int64_t Np, int64_t N,
                                                            const double* __restrict__ R, double* __restrict__ U) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double* __restrict__ rhs = R + (int64_t)blockIdx.y * Np;
    for (int e = 0; e < 16; e++) {
        const int64_t row = (int64_t)blockIdx.x * 64 + 16 * w + e;
        double v = 0.0;
        if (row < N) {
            for (int64_t c0 = 0; c0 <= row; c0 += 64) {
                const int64_t c = c0 + lane;
                if (c <= row) v = fma(V[row * Np + c], rhs[c], v);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) U[(int64_t)blockIdx.y * Np + row] = v;
    }
}

// the batch items of the engine launch B_k = Kf K_k, k = 0 .. d - 1 (offsets relative to Kf / Km / Bm)
__global__ void lml_hess_items_kernel(GemmBatchItem* __restrict__ items, int d, int64_t Np) {
    const int k = threadIdx.x;
    if (k >= d) return;
    GemmBatchItem it;
    it.a_off = 0; it.b_off = (int64_t)k * Np * Np; it.c_off = (int64_t)k * Np * Np;
    it.M = (int)Np; it.N = (int)Np; it.K = (int)Np; it.pad = 0;
    items[k] = it;
}

// grid: the lower-triangle tile pairs (ta >= tb); 256 threads.  G[mi][mj] = sum over the pairs (a, b) of tile (ta, tb) of
// B_mi[a, b] B_mj[b, a], matrix index m = 0: B_0 = I - Kf diag(alpha + w); 1 .. d: the engine's products; d + 1 (white):
// w Kf; above: zeros.  Lane (g, r) supplies matrices r, 16 + r, ... of the pair (a, b = 4 bq + g): the A operand from tile
// (ta, tb), the B operand from its mirror position in tile (tb, ta).  Wave w owns rows 16 w .. 16 w + 15 of the tile; the
// waves are combined as (w0 + w1) + (w2 + w3).  tpart[tile][MB * 16][MB * 16], row-major, NOT symmetric: the finish adds
// G + G^T (off-diagonal tile pairs: the mirror tile's pairs give the transposed Gram) or takes G alone (diagonal tiles).
template <int MB>
__global__ __launch_bounds__(256) void lml_hess_btraces_kernel(const double* __restrict__ Bm, const double* __restrict__ Kf, int64_t Np,
                                                               int64_t N, const double* __restrict__ noise, double white, int white_on,
                                                               int d, double* __restrict__ tpart) {
    constexpr int MBS = MB * 16;
    __shared__ double red[2 * MB * MB * 256];
    int ta, tb; lh_tri(blockIdx.x, &ta, &tb);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, g = lane >> 4, r = lane & 15;
    const int64_t sq = Np * Np;
    const double* base[MB];
    int type[MB];       // 0: zeros, 1: a stored product, 2: B_0, 3: B_w
#pragma unroll
    for (int b = 0; b < MB; b++) {
        const int m = b * 16 + r;
        base[b] = Kf; type[b] = 0;
        if (m == 0) type[b] = 2;
        else if (m <= d) { type[b] = 1; base[b] = Bm + (int64_t)(m - 1) * sq; }
        else if (m == d + 1 && white_on) type[b] = 3;
    }
    v4d acc[MB * MB];
#pragma unroll
    for (int b = 0; b < MB * MB; b++) acc[b] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int bq = 0; bq < 16; bq++) {
        const int64_t cb = (int64_t)tb * 64 + 4 * bq + g;
        const double n_b = cb < N ? noise[cb] + white : 0.0;
#pragma unroll 4
        for (int ar = 0; ar < 16; ar++) {
            const int64_t ca = (int64_t)ta * 64 + 16 * w + ar;
            const double n_a = ca < N ? noise[ca] + white : 0.0;
            const double dl = (ca == cb && ca < N) ? 1.0 : 0.0;
            double x[MB], y[MB];
#pragma unroll
            for (int b = 0; b < MB; b++) { x[b] = base[b][ca * Np + cb]; y[b] = base[b][cb * Np + ca]; }
#pragma unroll
            for (int b = 0; b < MB; b++) {
                if (type[b] == 2) { x[b] = dl - x[b] * n_b; y[b] = dl - y[b] * n_a; }
                else if (type[b] == 3) { x[b] *= white; y[b] *= white; }
                else if (type[b] == 0) { x[b] = 0.0; y[b] = 0.0; }
            }
#pragma unroll
            for (int p = 0; p < MB; p++)
#pragma unroll
                for (int q = 0; q < MB; q++)
                    acc[p * MB + q] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[p], y[q], acc[p * MB + q], 0, 0, 0);
        }
    }
    // (w0 + w1) + (w2 + w3): the odd waves hand theirs over, then wave 2 its sum
    double* mine = red + (w >> 1) * MB * MB * 256;
    if (w & 1) {
#pragma unroll
        for (int b = 0; b < MB * MB; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) mine[(b * 4 + q) * 64 + lane] = acc[b][q];
    }
    __syncthreads();
    if (!(w & 1)) {
#pragma unroll
        for (int b = 0; b < MB * MB; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[b][q] += mine[(b * 4 + q) * 64 + lane];
    }
    __syncthreads();
    if (w == 2) {
#pragma unroll
        for (int b = 0; b < MB * MB; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) red[(b * 4 + q) * 64 + lane] = acc[b][q];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int p = 0; p < MB; p++)
#pragma unroll
            for (int q2 = 0; q2 < MB; q2++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int b = p * MB + q2;
                    const double v = acc[b][q] + red[(b * 4 + q) * 64 + lane];
                    tpart[(int64_t)blockIdx.x * MBS * MBS + (p * 16 + g + 4 * q) * MBS + q2 * 16 + r] = v;
                }
    }
}

// Last kernel of an evaluation: workgroup e = (i <= j) of the upper triangle of H.  Three sums, each a strided pass of
// the 256 threads over its partial results in ascending order and the fixed LDS tree: the weighted Gram over the nb * nb
// tiles (two length scales), u_i . u_j over the rows, the pair trace over the tile pairs.  grad: the gradient as stage (a)
// left it on the device.  H_ij and its mirror image go straight into the mapped host buffer.
__global__ __launch_bounds__(256) void lml_hess_finish_kernel(const double* __restrict__ gpart, int64_t ntile2, int NB2,
                                                              const double* __restrict__ tpart, int64_t ntile, int MBS,
                                                              const double* __restrict__ U, int64_t Np, const double* __restrict__ grad,
                                                              int d, int white_on, int p, double* __restrict__ host_res) {
    __shared__ double red[256];
    int j, i; lh_tri(blockIdx.x, &j, &i);       // i <= j
    const int t = threadIdx.x;
    const bool ls_i = i >= 1 && i <= d, ls_j = j >= 1 && j <= d;
    double first = 0.0;
    if (i == 0) first = j <= d ? grad[j] : 0.0;                 // K_00 = K_0, K_0i = K_i; (log C, log w): 0
    else if (ls_i && ls_j) {
        const int a = j - 1, b = i - 1;                         // a >= b: the lower blocks
        const int blk = (a >> 4) + (b >> 4);                    // (0,0) -> 0, (1,0) -> 1, (1,1) -> 2
        const int off = (a & 15) * 16 + (b & 15);
        double s = 0.0;
        for (int64_t k = t; k < ntile2; k += 256) s += gpart[(k * NB2 + blk) * 256 + off];
        s = lh_block_sum(s, red);
        first = 0.5 * s - (i == j ? 2.0 * grad[i] : 0.0);
    } else if (i == j) first = grad[i];                         // (log w, log w); (log l, log w): 0
    double m = 0.0;
    for (int64_t k = t; k < Np; k += 256) m = fma(U[(int64_t)i * Np + k], U[(int64_t)j * Np + k], m);
    m = lh_block_sum(m, red);
    double tr = 0.0;
    for (int64_t k = t; k < ntile; k += 256) {
        int ta, tb; lh_tri(k, &ta, &tb);
        const double* G = tpart + k * MBS * MBS;
        const double v = G[i * MBS + j] + G[j * MBS + i];
        tr += ta == tb ? 0.5 * v : v;
    }
    tr = lh_block_sum(tr, red);
    if (t == 0) {
        const double h = (first - m) + 0.5 * tr;
        host_res[LH_HOFF + i * p + j] = h;
        host_res[LH_HOFF + j * p + i] = h;
    }
}

// Km[k] = dK / dlog l_k among the training rows, k < d: d full zero-padded squares of Np x Np doubles, from the scaled rows the
// context holds (the caller has called ensure_pred_xs) at the context's own theta -- the matrices of stage (b), by its kernel
int lml_hess_km_launch(gpry_ctx* ctx, double* Km) {
    const KernParams kp = make_kp(ctx);
    const int nb = (int)(ctx->Np / LH_T);
    const unsigned grid = (unsigned)(nb * nb);
#define LHK2(NBK, KID) hipLaunchKernelGGL((lml_hess_pairs_kernel<NBK, KID, true>), dim3(grid), dim3(256), 0, ctx->stream, ctx->dXs, \
                                          (const double*)nullptr, ctx->Np, (const double*)nullptr, Km, (double*)nullptr,       \
                                          (double*)nullptr, kp, nb)
#define LHK4(KID) { if (ctx->d <= 16) LHK2(1, KID); else LHK2(2, KID); }
    DISPATCH_KID(ctx->kernel_id, LHK4)
#undef LHK4
#undef LHK2
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

namespace {

// tile counts of the stages -- functions of the model size alone
struct LmlHessPlan {
    int nb, NB2, MB, nsplit, p;
    int64_t ntile;
};
LmlHessPlan lml_hess_plan(const gpry_ctx* ctx) {
    LmlHessPlan q;
    const int64_t Np = ctx->Np;
    const int d = ctx->d;
    q.p = ctx_ntheta(ctx);
    q.nb = (int)(Np / LH_T);
    q.ntile = (int64_t)q.nb * (q.nb + 1) / 2;
    q.NB2 = d <= 16 ? 1 : 3;            // accumulator tiles of the weighted Gram: one block of 16 coordinates, or two
    q.MB = (d + 2 + 15) / 16;           // matrix indices 0 .. d + 1
    // split-K of the batched product: only where the d * (Np / 128)^2 tiles leave most of the GPU idle
    q.nsplit = splitk_count((int64_t)d * (Np / 128) * (Np / 128), Np);
    return q;
}

// cs: the caller's claim of the call scratch, which it holds until it has waited for the chain
int lml_hess_chain(gpry_ctx* ctx, CallScratch& cs, double* dres) {
    const int64_t Np = ctx->Np, N = ctx->N, sq = Np * Np;
    const int d = ctx->d;
    const LmlHessPlan pl = lml_hess_plan(ctx);
    // The call scratch, claimed before the first launch: K^-1 as a full square, the d matrices K_i and K^-1 K_i, the partial
    // sums of the stages, the batch items of the product (one per length scale).  lml_chain and the GEMM engine work in the
    // objective's own buffers and claim nothing; what the factor chain queues on the side stream it joins into ctx->stream
    // before it returns, and nothing of the scratch is touched there.
    const auto rKf = cs.take<double>(sq), rKm = cs.take<double>(d * sq), rBm = cs.take<double>(d * sq),
               rgp = cs.take<double>((int64_t)pl.nb * pl.nb * pl.NB2 * 256), rmv = cs.take<double>((int64_t)pl.nb * d * Np),
               rR = cs.take<double>((int64_t)(d + 2) * Np), rU = cs.take<double>((int64_t)(d + 2) * Np),
               rtp = cs.take<double>(pl.ntile * (pl.MB * 16) * (pl.MB * 16));
    const auto ritems = cs.take<GemmBatchItem>(GPRY_MAX_DIM);
    GPRY_TRY(cs.claim());
    double *Kf = cs.at(rKf), *Km = cs.at(rKm), *Bm = cs.at(rBm), *gp = cs.at(rgp), *mv = cs.at(rmv), *R = cs.at(rR), *U = cs.at(rU),
           *tp = cs.at(rtp);
    GemmBatchItem* items = cs.at(ritems);
    hipStream_t st = ctx->stream;
    // (a) gpry_lml's chain with gradient -- the very function, hence its bits: L in dW, V in dW2, K^-1 (lower) in dW3, alpha and
    // [logdet/2, quad, grad ...] in dvec; value, gradient and status in gpry_lml's row of `dres`
    GPRY_TRY(lml_chain(ctx, 1, dres));
    double* da = ctx->dvec + Np;
    double* dout = ctx->dvec + 2 * Np;
    const KernParams kp = make_kp(ctx);
    {
        StageScope s(ctx, "hess_pairs");
        hipLaunchKernelGGL(lml_hess_mirror_kernel, dim3((unsigned)pl.ntile), dim3(256), 0, st, ctx->dW3, Np, N, Kf);
        const unsigned grid = (unsigned)(pl.nb * pl.nb);
#define LHP2(NBK, KID) hipLaunchKernelGGL((lml_hess_pairs_kernel<NBK, KID>), dim3(grid), dim3(256), 0, st, ctx->dXs, Kf, Np, da, Km, gp, mv, \
                                          kp, pl.nb)
#define LHP4(KID) { if (pl.NB2 == 1) LHP2(1, KID); else LHP2(2, KID); }
        DISPATCH_KID(ctx->kernel_id, LHP4)
#undef LHP4
#undef LHP2
        hipLaunchKernelGGL(lml_hess_items_kernel, dim3(1), dim3(64), 0, st, items, d, Np);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        // (c) B_k = Kf K_k: one batched launch of the engine
        StageScope s(ctx, "hess_products");
        GemmArgs g = {};
        g.A = Kf; g.lda = Np; g.B = Km; g.ldb = Np; g.C = Bm; g.ldc = Np;
        g.M = (int)Np; g.N = (int)Np; g.K = (int)Np;
        g.kmode = KM_FULL; g.lower_only = 0; g.tile_map = TM_ROWMAJOR; g.info = ctx->dinfo;
        g.batch = items; g.n_batch = d; g.dma_ok = 1;
        if (pl.nsplit > 1) {
            // (asked for here, not up front: the factor chain asks for slices of its own and may have replaced the buffer)
            double* sbuf = nullptr;
            GPRY_TRY(gemm_split_scratch(ctx, pl.nsplit, (int64_t)d * Np * Np, &sbuf));
            g.nsplit = pl.nsplit; g.split_buf = sbuf; g.split_stride = (int64_t)d * Np * Np;
        }
        g.small64 = 1;          // Np is a multiple of 128
        GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
    }
    {
        StageScope s(ctx, "hess_btraces");
        if (pl.MB == 1)
            hipLaunchKernelGGL(lml_hess_btraces_kernel<1>, dim3((unsigned)pl.ntile), dim3(256), 0, st, Bm, Kf, Np, N, ctx->dnoise, kp.white,
                               kp.white_on, d, tp);
        else if (pl.MB == 2)
            hipLaunchKernelGGL(lml_hess_btraces_kernel<2>, dim3((unsigned)pl.ntile), dim3(256), 0, st, Bm, Kf, Np, N, ctx->dnoise, kp.white,
                               kp.white_on, d, tp);
        else
            hipLaunchKernelGGL(lml_hess_btraces_kernel<3>, dim3((unsigned)pl.ntile), dim3(256), 0, st, Bm, Kf, Np, N, ctx->dnoise, kp.white,
                               kp.white_on, d, tp);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        StageScope s(ctx, "hess_middle");
        hipLaunchKernelGGL(lml_hess_rhs_kernel, dim3((unsigned)((Np + 255) / 256), (unsigned)pl.p), dim3(256), 0, st, mv, ctx->dy,
                           ctx->dnoise, da, Np, N, d, pl.nb, kp.white, R);
        hipLaunchKernelGGL(lml_hess_trmv_kernel, dim3((unsigned)pl.nb, (unsigned)pl.p), dim3(256), 0, st, ctx->dW2, Np, N, R, U);
        HIP_TRY(ctx, hipGetLastError());
    }
    StageScope s(ctx, "hess_finish");
    hipLaunchKernelGGL(lml_hess_finish_kernel, dim3((unsigned)(pl.p * (pl.p + 1) / 2)), dim3(256), 0, st, gp, (int64_t)pl.nb * pl.nb,
                       pl.NB2, tp, pl.ntile, pl.MB * 16, U, Np, dout + 2, d, kp.white_on, pl.p, dres);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int gpry_lml_hessian(gpry_ctx* ctx, const double* theta, double* lml, double* grad, double* hess, int* info, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_lml_hessian: ctx is NULL");
    if (!theta || !lml || !grad || !hess || !info)
        return gpry_fail(ctx, -1, "lml_hessian: theta, lml, grad, hess and info must not be NULL");
    GPRY_TRY(objective_entry(ctx, "lml_hessian", theta, 1));
    if (ctx->Np > LH_MAX_NP)
        return gpry_fail(ctx, -1, "lml_hessian: %lld padded rows exceed the limit of %d", (long long)ctx->Np, LH_MAX_NP);
    double *hres, *dres;
    GPRY_TRY(objective_row(ctx, 8 * (LH_HOFF + GPRY_THETA_MAX * GPRY_THETA_MAX), LH_INFO, &hres, &dres));
    ThetaScope at(ctx, theta);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int rc = 0;
    if (device_ms) {
        if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess || hipEventRecord(ev0, ctx->stream) != hipSuccess)
            rc = gpry_fail(ctx, -2, "lml_hessian: no timing events");
    }
    // Where gpry_lml answers from its single launch (N <= 128, d <= 16), value and gradient come from that launch here too:
    // the caller gets gpry_lml's bits at every size.  The Hessian takes the chain at 128 padded rows and builds its row of
    // log C and the -2 grad_i of its diagonal from the CHAIN's gradient, which agrees with the returned one to rounding:
    // for such a model H[0][j] == grad[j] holds to rounding, not to the bit.
    bool fused = false;
    double fhost[2 + GPRY_THETA_MAX];
    int finfo = 0, cinfo = 0;
    if (rc == 0 && ctx->opt_lml_small && ctx->opt_chol == 0) {
        StageScope s(ctx, "lml_small");
        const int r = launch_lml_small(ctx, 1, fhost, &finfo);
        if (r < 0) rc = r;
        fused = r == 0;
    }
    const bool ran = rc == 0 && !(fused && finfo != 0);
    CallScratch cs(ctx, "gpry_lml_hessian");
    if (ran) {
        rc = lml_hess_chain(ctx, cs, dres);
        at.factor_chain_ran();
    }
    if (ev1 && rc == 0) (void)hipEventRecord(ev1, ctx->stream);
    rc = objective_wait(ctx, "lml_hessian", rc, ran ? hres : nullptr, LH_INFO, &cinfo);
    float ms = 0.0f;
    if (ev0 && ev1 && rc == 0) (void)hipEventElapsedTime(&ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (device_ms) *device_ms = (double)ms;
    if (rc) return rc;
    *info = finfo != 0 ? finfo : cinfo;
    objective_write(ctx, *info, lml_head(fused ? fhost : hres), (fused ? fhost : hres) + 2, hres + LH_HOFF, lml, grad, hess);
    return 0;
}

}  // extern "C"
