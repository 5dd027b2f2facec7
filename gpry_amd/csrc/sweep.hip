// The candidate sweep: posterior mean, sigma and LogExp acquisition of a pool of candidates in chunks (gpry_sweep_logexp,
// gpry_sweep_logexp_given, the panel paths of gpry_predict), stage A and the compact batches of a pruned sweep.
#include "sweep.h"
#include "acq_math.h"
#include <algorithm>

__global__ void logexp_kernel(const double* __restrict__ mu, const double* __restrict__ sd, int64_t n, double zeta,
                              double baseline, double sigma_n, double* __restrict__ acq) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acq[i] = logexp_value(mu[i], sd[i], zeta, baseline, sigma_n);
}
int launch_logexp(gpry_ctx* ctx, const double* mu, const double* sd, int64_t n, double zeta, double baseline, double sigma_n, double* acq) {
    hipLaunchKernelGGL(logexp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, sd, n, zeta, baseline, sigma_n, acq);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// THE FINISH, once: every finish kernel below takes y, sigma and the prior sigma from finish_y below and finish_sd /
// logexp_value of acq_math.h, so that a candidate gets
// the same operations on the same values -- the same bits -- whichever kernel finishes it.  The exactness of the pruned sweep
// rests on that (ub >= acq bit for bit, y of a contracted candidate = y of the full sweep).
// The per-tile partials of column `col`, added in ascending tile order from 0.0
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nt, int64_t ldp, int64_t col) {
    double s = 0.0;
#pragma unroll 8
    for (int t = 0; t < nt; t++) s += part[(int64_t)t * ldp + col];
    return s;
}
// y of the normalised mean mu_: the reference's post-processing chain (gpry/gpr.py:1180-1231); -inf under any mask bit
__device__ __forceinline__ double finish_y(double mu_, unsigned mk, const FinishParams& fp) {
    double y = mu_ * fp.y_std + fp.y_mean;
    y = fmin(y, fp.clip_hi);
    if (mk) y = -INFINITY;
    return y;
}
// per candidate: reduce the partials, apply the reference's post-processing chain
// (gpry/gpr.py:1180-1231) and LogExp.f (gpry/acquisition_functions.py:1068-1074)
__global__ void sweep_finish_kernel(const double* __restrict__ mean_part, const double* __restrict__ ss_part,
                                    int nt_mean, int nt, int64_t ldp, int64_t m0, int64_t mc, const uint8_t* __restrict__ mask,
                                    double* __restrict__ y_all, double* __restrict__ sig_all,
                                    double* __restrict__ acq_all, FinishParams fp) {
    int64_t ml = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ml >= mc) return;
    int64_t m = m0 + ml;
    const double mu_ = sum_partials(mean_part, nt_mean, ldp, ml);
    const unsigned mk = mask ? mask[m] : 0u;
    const double y = finish_y(mu_, mk, fp);
    y_all[m] = y;
    if (!fp.want_std) return;
    const double ss = sum_partials(ss_part, nt, ldp, ml);
    const double sd = finish_sd(ss, mk, fp);
    sig_all[m] = sd;
    if (!fp.want_acq) return;
    acq_all[m] = logexp_value(y, sd, fp.zeta, fp.baseline, fp.sigma_n);
}

// The finish of a sweep whose y the caller supplied (gpry_sweep_logexp_given; the reference's mpi.compute_y_parallel with y
// given and sigma_y None, gpry/mpi.py:182-218 -> gpr.predict_std, gpry/gpr.py:1275-1352): y is the caller's, already in
// y_all, and is neither mapped, clipped nor masked; sigma and acq are sweep_finish_kernel's (finish_sd on the same per-tile
// sums in the same order), so sigma is bit for bit the ordinary sweep's.
__global__ void sweep_given_finish_kernel(const double* __restrict__ ss_part, int nt, int64_t ldp, int64_t m0, int64_t mc,
                                          const uint8_t* __restrict__ mask, const double* __restrict__ y_all,
                                          double* __restrict__ sig_all, double* __restrict__ acq_all, FinishParams fp) {
    int64_t ml = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ml >= mc) return;
    int64_t m = m0 + ml;
    const unsigned mk = mask ? mask[m] : 0u;
    const double ss = sum_partials(ss_part, nt, ldp, ml);
    const double sd = finish_sd(ss, mk, fp);
    sig_all[m] = sd;
    acq_all[m] = logexp_value(y_all[m], sd, fp.zeta, fp.baseline, fp.sigma_n);
}

// Stage A of a pruned sweep: y exactly as sweep_finish_kernel computes it, and the acquisition the candidate would have with
// ss = 0 (the prior sigma) -- an upper bound of its exact value, bit for bit (finish_sd); y and the linear term are the same
// operations on the same values.  acq_all starts as the bound, sig_all as PRUNED_SIGMA; the contracted candidates overwrite
// both (sweep_scatter_finish_kernel).
__global__ void sweep_mean_kernel(const double* __restrict__ mean_part, int nt_mean, int64_t ldp, int64_t m0, int64_t mc,
                                  const uint8_t* __restrict__ mask, double* __restrict__ y_all, double* __restrict__ sig_all,
                                  double* __restrict__ acq_all, double* __restrict__ ub, FinishParams fp) {
    int64_t ml = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ml >= mc) return;
    int64_t m = m0 + ml;
    const double mu_ = sum_partials(mean_part, nt_mean, ldp, ml);
    const unsigned mk = mask ? mask[m] : 0u;
    const double y = finish_y(mu_, mk, fp);
    y_all[m] = y;
    const double sd = finish_sd(0.0, mk, fp);
    const double a = logexp_value(y, sd, fp.zeta, fp.baseline, fp.sigma_n);
    ub[m] = a;
    acq_all[m] = a;
    sig_all[m] = PRUNED_SIGMA;
}

// Stage A of a pruned sweep with the bound pass (option "sweep_mean_bound"; mean_bound_setup explains the slack D1 + g3 * S): an
// upper bound of y instead of y, the same finish behind it.  Each candidate's bound partials are summed as the exact partials
// are (same order), the slack is added and the sum rounded up; y = mu * y_std + y_mean, the clip, and every step behind them
// to the acquisition are monotone in mu under round-to-nearest (y_std > 0, zeta >= 0), masks give -inf as in
// sweep_mean_kernel, and NaN comes out exactly where the exact y is NaN (a NaN term is never skipped).  y_all holds the bound
// until the candidate is contracted (sweep_scatter_finish_kernel with mean partials writes the exact y).
__global__ void sweep_mean_bound_kernel(const double* __restrict__ mean_part, const double* __restrict__ sabs_part, int nt_mean,
                                        int64_t ldp, int64_t m0, int64_t mc, const uint8_t* __restrict__ mask,
                                        double* __restrict__ y_all, double* __restrict__ sig_all, double* __restrict__ acq_all,
                                        double* __restrict__ ub, FinishParams fp, double D1, double g3) {
    int64_t ml = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ml >= mc) return;
    int64_t m = m0 + ml;
    double mu_ = sum_partials(mean_part, nt_mean, ldp, ml);
    const double sa = sum_partials(sabs_part, nt_mean, ldp, ml);
    mu_ = nextafter(mu_ + (D1 + g3 * sa), INFINITY);
    const unsigned mk = mask ? mask[m] : 0u;
    const double y = finish_y(mu_, mk, fp);
    y_all[m] = y;
    const double sd = finish_sd(0.0, mk, fp);
    const double a = logexp_value(y, sd, fp.zeta, fp.baseline, fp.sigma_n);
    ub[m] = a;
    acq_all[m] = a;
    sig_all[m] = PRUNED_SIGMA;
}

// Stage A of a pruned sweep whose y the caller supplied (gpry_sweep_logexp_given): it replaces the mean pass -- no panel, no
// cross build, no candidate centring.  ub = acq_all = the acquisition at the caller's y and the prior sigma (0 on classifier-
// inf rows, as the finish gives them), sig_all = PRUNED_SIGMA.  The bound holds bit for bit by the argument at finish_sd
// (the finish: sweep_given_finish_kernel, sweep_scatter_finish_kernel); y and the linear term are the same operations on
// the same values.
__global__ void sweep_given_bound_kernel(int64_t m0, int64_t mc, const uint8_t* __restrict__ mask,
                                         const double* __restrict__ y_all, double* __restrict__ sig_all,
                                         double* __restrict__ acq_all, double* __restrict__ ub, FinishParams fp) {
    int64_t ml = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ml >= mc) return;
    int64_t m = m0 + ml;
    const unsigned mk = mask ? mask[m] : 0u;
    const double sd = finish_sd(0.0, mk, fp);
    const double a = logexp_value(y_all[m], sd, fp.zeta, fp.baseline, fp.sigma_n);
    ub[m] = a;
    acq_all[m] = a;
    sig_all[m] = PRUNED_SIGMA;
}

// The finish of a compact batch (pool indices gidx[0..n)): sigma and acq as sweep_finish_kernel computes them from the same
// per-tile partials, summed in the same order, with the y stage A stored -- or, after the bound pass (mean_part != NULL), y
// from the batch's own mean partials as sweep_finish_kernel computes it (stored over the bound)
__global__ void sweep_scatter_finish_kernel(const double* __restrict__ ss_part, int nt, int64_t ldp, const int64_t* __restrict__ gidx,
                                            int64_t n, const uint8_t* __restrict__ mask, double* __restrict__ y_all,
                                            double* __restrict__ sig_all, double* __restrict__ acq_all, FinishParams fp,
                                            const double* __restrict__ mean_part) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t m = gidx[i];
    if (mean_part) {
        const double mu_ = sum_partials(mean_part, nt, ldp, i);
        y_all[m] = finish_y(mu_, mask ? mask[m] : 0u, fp);
    }
    const double ss = sum_partials(ss_part, nt, ldp, i);
    const double sd = finish_sd(ss, mask ? mask[m] : 0u, fp);
    sig_all[m] = sd;
    acq_all[m] = logexp_value(y_all[m], sd, fp.zeta, fp.baseline, fp.sigma_n);
}

// rows gidx[0..n) of the pool, then zero rows up to n_pad (the panel builders read whole 256-row blocks)
__global__ void gather_rows_kernel(const double* __restrict__ Xc, int d, const int64_t* __restrict__ gidx, int64_t n,
                                   int64_t n_pad, double* __restrict__ Xg) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pad * d) return;
    const int64_t i = e / d;
    const int k = (int)(e - i * d);
    Xg[e] = i < n ? Xc[gidx[i] * d + k] : 0.0;
}

// Split-K contraction of a small batch: the slices P[y] (Np x ldp each, `stride` doubles apart) hold
// partial products of u = V k*; per 128-row tile ti and candidate m
//     ss_part[ti][m] = sum_{i in tile} ( sum_y P[y][i][m] )^2
// -- the same per-tile partials the SUMSQ epilogue of the one-pass contraction leaves, slices added
// in a fixed order (deterministic).  Block = one row tile x 64 candidates, 4 waves x 32 rows.
template <int NS>
__global__ __launch_bounds__(1024) void splitk_sumsq_kernel(const double* __restrict__ P, int64_t stride,
                                                            int64_t ldp, double* __restrict__ ss_part) {
    // 1024 threads = 64 candidates x 16 row groups of 8 rows: every thread has its NS x 2 loads of two
    // rows in flight at once (a 256-thread version that walked 32 rows x NS slices per thread was a
    // chain of dependent memory round trips: 100+ us for a 20-us amount of data)
    __shared__ double red[16][64];
    const int ti = blockIdx.x, col = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.y * 64 + col;
    double acc = 0.0;
#pragma unroll
    for (int rr = 0; rr < 8; rr += 2) {
        const int64_t off = ((int64_t)ti * 128 + rg * 8 + rr) * ldp + c;
        double v0[NS], v1[NS];
#pragma unroll
        for (int y = 0; y < NS; y++) { v0[y] = P[(int64_t)y * stride + off]; v1[y] = P[(int64_t)y * stride + off + ldp]; }
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int y = 0; y < NS; y++) { u0 += v0[y]; u1 += v1[y]; }      // slices in a fixed order
        acc = fma(u0, u0, acc);
        acc = fma(u1, u1, acc);
    }
    red[rg][col] = acc;
    __syncthreads();
    if (rg == 0) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) s += red[k][col];
        ss_part[(int64_t)ti * ldp + c] = s;
    }
}

// the correlation at the scaled argument u = corr_scale * r^2 (kern_math.h: corr_scaled_fast), from libm
static double corr_scaled_host(int kid, double u) {
    if (kid == GPRY_RBF) return exp(-u);
    const double t = sqrt(u);
    if (kid == GPRY_MATERN12) return exp(-t);
    if (kid == GPRY_MATERN32) return (1.0 + t) * exp(-t);
    return (1.0 + t + t * t / 3.0) * exp(-t);
}

static int ensure_sweep_buffers(gpry_ctx* ctx, int64_t M) {
    if (M > ctx->sw_cap) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        void* old[] = {ctx->dXc, ctx->dmask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all};
        for (void* p : old) if (p) GPRY_TRY(dev_free(ctx, p));
        int64_t cap = round_up(M, 1024);
        GPRY_TRY(dev_alloc(ctx, &ctx->dXc, cap * GPRY_MAX_DIM));
        GPRY_TRY(dev_alloc(ctx, &ctx->dmask, cap));
        GPRY_TRY(dev_alloc(ctx, &ctx->dy_all, cap));
        GPRY_TRY(dev_alloc(ctx, &ctx->dsig_all, cap));
        GPRY_TRY(dev_alloc(ctx, &ctx->dacq_all, cap));
        ctx->sw_cap = cap;
    }
    return 0;
}

// candidates per chunk: the K* panel of a chunk (Np x chunk doubles) is 1 GiB at Np = 4096 and stays that size for smaller
// models -- at Np = 1024 the 1e5 candidates of BASELINE configs[1] are ONE launch of 6256 tiles instead of three and a
// ragged fourth (contraction 0.60 -> 0.71 of peak); a candidate's result does not depend on the chunking
static int64_t sweep_chunk(const gpry_ctx* ctx, int64_t M) {
    int64_t chunk = ctx->opt_sweep_chunk;
    if (chunk <= 0) chunk = ctx->Np < 4096 ? round_up(32768 * 4096 / ctx->Np, 1024) : 32768;
    if (chunk > round_up(M, 128)) chunk = round_up(M, 128);
    return chunk;
}

// THE PANEL FORM of a sweep / panel predict: sets ctx->panel_form (the codes at its declaration) and ctx->panel_est.
// small_build: gpry_predict with a few hundred points, whose panel comes from the small-batch kernel.
static bool panel_from_matrix_pipe(int form) { return form == 1 || form == 4; }
static int choose_panel_form(gpry_ctx* ctx, bool small_build) {
    // distances of the panel from the matrix pipe (cross_build_mfma_kernel; "cross_mfma" = 0: the difference form)
    // (not for Matern-1/2: exp(-r) has a cusp at r = 0, where the rounding noise e of the expanded r^2 becomes sqrt(e) in r --
    // 1e-7 in k for a candidate on a training point; the smoother kernels see e itself)
    bool fast_panel = ctx->opt_cross_mfma && !small_build && ctx->kernel_id != GPRY_MATERN12;
    bool hybrid_panel = false;
    ctx->panel_form = small_build ? 3 : 2;
    ctx->panel_est[0] = ctx->panel_est[1] = ctx->panel_est[2] = 0.0; ctx->panel_est[3] = 2.5e-7;
    if (!fast_panel) return 0;
    // ... and not for a model that would amplify that noise beyond the posterior tolerance.  The expanded form has
    // |d r^2| <= 4 eps (|x - c|^2 + |y - c|^2) <= 4 eps (2 r^2 + 4 R^2), with R^2 the largest |y - c|^2 of a training row
    // (bounded below by the per-dimension extent of the training set) -- whatever the candidate: a far one has a large
    // r^2, and r^2 |dk / d r^2| <= C / 2, |dk / d r^2| <= 1.5 C for the three smooth kernels.  Every entry of K* is thus
    // off by at most e = 4 eps C (1 + 6 R^2) -- attained only by a candidate that sits on a training row at the rim of
    // the set; a random candidate sees a small fraction of it.
    //   * MEAN = k*^T alpha_: at worst e ||alpha_||_1 (est[1], reported); the rounding errors of different pairs being
    //     independent, in effect e ||alpha_||_2 (est[0], gated).
    //   * VARIANCE = C - ||V k*||^2: d var = -2 w^T dk with w = K^-1 k*, i.e. 2 e ||w||_2 in the same statistical sense.
    //     ||w||_2^2 = k*^T K^-2 k* <= ||K^-1||_2 k*^T K^-1 k* <= C / lambda_min(K) (the posterior variance is >= 0), and
    //     lambda_min(K) >= the smallest noise variance on the diagonal: ||w||_2 <= sqrt(C) / sigma_n,min for EVERY
    //     candidate (typical candidates have ||w||_2 = O(1); the bound is attained by a k* along the weakest eigenvector).
    //     Relative to C: est[2] = 2 e / (sigma_n,min sqrt(C)).  (Round 6: until then the gate had no variance term.)
    // Both are held below 2.5e-7 (est[3]) -- of the unit-variance normalised targets, resp. of the prior variance C --, a
    // quarter of the 1e-6 the posterior is specified to; on well-conditioned models they are 1e-12 ... 1e-10 (the parity
    // tests compare at 1e-8 / 1e-9 C).  A nearly singular K (tiny noise, long length scales: large alpha_) or length
    // scales far below the extent of the training set (large R^2) take the difference form, whose entries are good to
    // 1e-15 C.  (BASELINE configs[2] as the bench fits it -- several length scales at their lower bound of 1e-3, R^2 =
    // 4e5, ||alpha_||_2 = 64 -- comes to 1.3e-7 for the mean and, since round 6, fails on the variance term.)
    if (ctx->alpha_l2 < 0.0) {
        std::vector<double> ha((size_t)ctx->N);
        HIP_TRY(ctx, hipMemcpyAsync(ha.data(), ctx->dalpha_, sizeof(double) * ctx->N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        double ss = 0.0, s1 = 0.0;
        for (double v : ha) { ss += v * v; s1 += fabs(v); }
        ctx->alpha_l2 = sqrt(ss); ctx->alpha_l1 = s1;
    }
    double R2 = 0.0;
    for (int k = 0; k < ctx->d; k++) {
        const double a = ctx->xhi[k] - ctx->xcenter[k], b = ctx->xcenter[k] - ctx->xlo[k];
        const double r = (a > b ? a : b) * exp(-ctx->theta[1 + k]);
        R2 += r * r;
    }
    const double C = exp(ctx->theta[0]);
    const double e = 4.0 * 2.220446049250313e-16 * C * (1.0 + 6.0 * R2);
    ctx->panel_est[0] = e * ctx->alpha_l2;
    ctx->panel_est[1] = e * ctx->alpha_l1;
    const double lam_min = ctx->noise_min + ctx_white(ctx);      // lambda_min(K) >= min(alpha) + w
    ctx->panel_est[2] = lam_min > 0.0 ? 2.0 * e / (sqrt(lam_min) * sqrt(C)) : INFINITY;
    if (!(ctx->panel_est[0] <= ctx->panel_est[3]) || !(ctx->panel_est[2] <= ctx->panel_est[3])) fast_panel = false;
    if (ctx->opt_panel_debug & 32) fast_panel = true;       // test hook: the matrix-pipe form whatever the estimates say
    if (fast_panel) ctx->panel_form = 1;
    // THE HYBRID FORM (round 6; cross_build_mfma_kernel<.., HYB>): distances from the matrix pipe, and every pair that comes
    // out nearer than r^2 = 100 -- the only ones whose kernel value listens to r^2 at the 1e-15 level -- again from the
    // coordinates, as the difference form does.  Its entries are as good as the difference form's; what decides between the
    // two is cost: a model that failed the gate through R^2 (length scales far below the extent of the data: the bench's
    // fitted model) has next to no near pairs and pays the matrix-pipe price; one that failed it through its weights at
    // ordinary length scales has nothing else and takes the difference form.
    else if (ctx->opt_cross_hybrid && R2 >= 1000.0) { hybrid_panel = true; ctx->panel_form = 4; }
    if (getenv("GPRY_HIP_DEBUG_PANEL")) {
        fprintf(stderr, "gpry: panel form: C %.3g R2 %.3g |alpha|_2 %.3g |alpha|_1 %.3g min noise %.3g -> mean %.3g (l1 %.3g) var %.3g: %s; l =", C, R2,
                ctx->alpha_l2, ctx->alpha_l1, ctx->noise_min, ctx->panel_est[0], ctx->panel_est[1], ctx->panel_est[2],
                fast_panel ? "matrix pipe" : hybrid_panel ? "hybrid" : "difference form");
        for (int k = 0; k < ctx->d; k++) fprintf(stderr, " %.3g (%.3g..%.3g)", exp(ctx->theta[1 + k]), ctx->xlo[k], ctx->xhi[k]);
        fprintf(stderr, "\n");
    }
    return 0;
}

// THE BOUND PASS (option "sweep_mean_bound"; stage A of a pruned sweep in the hybrid form, cross_build_mfma_kernel<.., BND>).
// The hybrid form is taken by models with length scales far below the extent of their data, whose candidates have next to
// no training row nearby: the pass skips every block of 16 rows x 32 candidates whose expanded u all lie in [ubnd, uhi]
// and sums the terms alpha_j v_j of the other blocks, each one the exact pass's to the bit (same code).  y is bounded by
//   * D = 2 C ||alpha_||_1 k(ubnd) >= the skipped terms in all: ubnd >= the hybrid form's cut, so the exact pass takes
//     those pairs' u as it is, and its v = C corr_scaled_fast(u) is within a few ulps of C k(u) <= C k(ubnd) up to
//     t = sqrt(u) = 763 (Matern) and 0 beyond (kern_math.h: the exponential underflows through ldexp; uhi keeps the
//     argument reduction exact, t <= 1e6).  ubnd is chosen for D = 1e-13 of the normalised targets.
//   * rounding: the exact y and the bound's partial sum are recursive sums of depth <= n = 128 rows + Np / 128 partials
//     + 4 (the shuffles), so each is within gamma = n eps of its exact value times the sum of |terms|.  With S the
//     (computed) sum of |alpha_j v_j| over the live terms:  y <= y_part + (1 + gamma) D + 2 gamma S (1 + gamma)
//     <= y_part + (1 + 2 gamma) D + 3 gamma S -- the slack, added and rounded up (sweep_mean_bound_kernel).
// A bound only moves the candidate up the ranking (more survivors); it never changes a record.  Not taken for a model
// whose weights or scales are not finite, y_std <= 0 or zeta < 0 (the acquisition would not be monotone in y).
// THE SCREEN (option "sweep_screen", kernel_build.hip) skips a block before that test where u32 = fmaf(-2 s, dot32,
// fl32(xn + yn)) of every pair lies in [ubnd + delta, uhi - delta]; it certifies only blocks the FP64 test would skip, so the
// skipped set is a subset of the one above and nothing in this proof changes.  delta bounds |u32 - u| for the u of the FP64
// test, with e = 2^-24, a = |x'|, b = |y'| (centred scaled, a b <= (a + b)^2 / 4, a^2 + b^2 <= (a + b)^2):
//   * the FP32 images move each coordinate by a factor 1 + e at most: the exact dot product of the images is within
//     (2 e + e^2) a b of x'.y', which is <= 4.1 e s a b in -2 s x'.y', i.e. <= 1.03 e s (a + b)^2;
//   * dot32 is a fmaf chain over the d coordinates that are not padding (zero products round nothing): within
//     gamma_d sum |x~ y~| <= 1.01 d e a b of that exact product, <= 0.51 d e s (a + b)^2 after the factor 2 s;
//   * fl32(xn + yn) rounds the FP64 sum once, <= e s (a^2 + b^2) (1 + 2^-50) <= 1.01 e s (a + b)^2; the last fmaf rounds once,
//     <= e |u32| <= 1.01 e s (a + b)^2 (|u32| <= s (a + b)^2 (1 + d e));
//   * the FP64 u itself is within 4 * 2^-53 s (a^2 + b^2) of the exact value (kernel_build.hip), 1e-8 of the terms above.
// In all <= (d / 2 + 3.1) e s (a + b)^2; delta = e (d + 8) s (max b + max a)^2, the maxima over the workgroup's rows and
// the wave's candidates, has more than twice that, which also covers the FP64 roundings of delta and the two thresholds
// themselves (these are then rounded inwards to FP32), and FP32 underflow: at most 2^-149 per operation, times a + b, where a
// certified block has s (a + b)^2 >= ubnd >= 50 and so delta > 2e-5.  No FP32 value overflows: the screen is off for a wave whose norms
// exceed 1e36 or are not finite.
struct MeanBound { bool on = false; double ubnd = 0.0, uhi = 0.0, D1 = 0.0, g3 = 0.0; };
static MeanBound mean_bound_setup(const gpry_ctx* ctx, const SweepRequest& rq, const FinishParams& fp, int nt) {
    MeanBound b;
    b.uhi = ctx->kernel_id == GPRY_RBF ? 1e6 : 1e12;
    if (rq.kind != SWEEP_STAGE_A || rq.y_given || ctx->panel_form != 4 || !ctx->opt_sweep_mean_bound) return b;
    const double C = exp(ctx->theta[0]), a1 = ctx->alpha_l1;
    const double sc = ctx->kernel_id == GPRY_RBF ? 0.5 : ctx->kernel_id == GPRY_MATERN32 ? 3.0 : 5.0;    // corr_scale
    const double scale = 2.0 * C * a1, target = 1e-13;
    if (!(std::isfinite(C) && C > 0.0 && std::isfinite(a1) && fp.y_std > 0.0 && std::isfinite(fp.y_std) && rq.zeta >= 0.0 &&
          scale * corr_scaled_host(ctx->kernel_id, b.uhi) <= target)) return b;
    double lo = 100.0 * sc, hi = b.uhi;
    if (scale * corr_scaled_host(ctx->kernel_id, lo) <= target) hi = lo;
    for (int it = 0; it < 200 && hi > lo * (1.0 + 1e-9); it++) {
        const double mid = sqrt(lo * hi);
        if (scale * corr_scaled_host(ctx->kernel_id, mid) <= target) hi = mid; else lo = mid;
    }
    b.ubnd = hi;
    const double D = scale * corr_scaled_host(ctx->kernel_id, b.ubnd);
    const double gamma = (double)(128 + nt + 4) * 2.220446049250313e-16;
    b.D1 = (1.0 + 2.0 * gamma) * D;
    b.g3 = 3.0 * gamma;
    b.on = true;
    return b;
}

// THE place that picks the panel launcher for a form code: columns [m0, m0 + ncols) of the candidates X into Kst (k-major,
// ld = ncols; NULL: not stored) and their mean partials into mean_part (NULL: none).  run_sweep and prune_eval both build
// through it, so a candidate's panel column and mean partials are the same bits in a compact batch as in the full sweep.
static int build_sweep_panel(gpry_ctx* ctx, int form, const double* X, int64_t m0, int64_t ncols, double* Kst, double* mean_part) {
    if (form == 3) return launch_cross_build_small(ctx, X, m0, ncols, ncols, Kst, mean_part, 1);
    if (panel_from_matrix_pipe(form)) return launch_cross_build_mfma(ctx, X, m0, ncols, ncols, Kst, mean_part, 1, form == 4 ? 1 : 0);
    return launch_cross_build(ctx, X, m0, ncols, ncols, Kst, mean_part, 1);
}
// THE one-pass contraction ss_part[ti][m] = sum_{i in tile ti} (V k*_m)_i^2 of a panel of ncols columns, for run_sweep and
// prune_eval alike: the k walk per row tile is a function of the row tile and Np alone, whoever launches it.
static int contract_sweep(gpry_ctx* ctx, const double* Kst, int64_t ncols, double* ss_part) {
    GemmArgs g = {};
    g.A = ctx->dV; g.lda = ctx->Np; g.B = Kst; g.ldb = ncols; g.C = ss_part; g.ldc = ncols;
    g.M = (int)ctx->Np; g.N = (int)ncols; g.K = (int)ctx->Np;
    g.kmode = KM_A_LOWER; g.lower_only = 0; g.tile_map = TM_SWEEP | (3 << 4);     // super-tiles of 8 row tiles x 8 candidate tiles
    if (ctx->opt_sweep_small_map) g.tile_map |= TM_SWEEP_SMALL;                   // (a launch of few tiles: one workgroup per tile)
    // LDS-DMA staging + software pipeline (sweep_gemm.hip); "gemm_dma" = 0: the register-staged engine (comparator)
    if (ctx->opt_gemm_dma) return sweep_gemm_dma_sp_launch(ctx, g);
    return gemm_f64_launch(ctx, g, false, false, EPI_SUMSQ);
}
// A batch of a few hundred to a few thousand points has fewer tiles than the GPU has workgroup
// slots, and its longest tile walks all Np/16 slabs alone (1 ms at Np = 4096): split every
// tile's k-range over grid.y so that ~512 workgroups share the contraction, keep the partial
// products u_y in scratch and square their sum in a second, small kernel.
// Only for gpry_predict: the NORA sweep keeps the one-pass contraction, whose result for a candidate
// does not depend on which other candidates share its launch -- a pool sharded over several
// contexts / GPUs then gives bit for bit what one context gives (tests/test_group_gpu.py).
static int predict_nsplit(const gpry_ctx* ctx, int64_t ncols) {
    const int64_t tiles = (ctx->Np / 128) * (ncols / 128);
    int nsplit = 1;
    while (nsplit < 16 && tiles * nsplit * 2 <= 1024 && ctx->Np / (nsplit * 2) >= 64) nsplit *= 2;
    return nsplit;
}
static int contract_splitk(gpry_ctx* ctx, const double* Kst, int64_t ncols, int nsplit, double* ss_part) {
    const int64_t Np = ctx->Np;
    double* sbuf = nullptr;
    GPRY_TRY(gemm_split_scratch(ctx, nsplit, Np * ncols, &sbuf));
    GemmArgs g = {};
    g.A = ctx->dV; g.lda = Np; g.B = Kst; g.ldb = ncols; g.C = sbuf; g.ldc = ncols;
    g.M = (int)Np; g.N = (int)ncols; g.K = (int)Np;
    g.kmode = KM_A_LOWER; g.tile_map = TM_ROWMAJOR;
    g.nsplit = nsplit; g.split_buf = sbuf; g.split_stride = Np * ncols; g.skip_reduce = 1;
    GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
    const dim3 rg((unsigned)(Np / 128), (unsigned)(ncols / 64));
    switch (nsplit) {
        case 2: hipLaunchKernelGGL(splitk_sumsq_kernel<2>, rg, dim3(1024), 0, ctx->stream, sbuf, Np * ncols, ncols, ss_part); break;
        case 4: hipLaunchKernelGGL(splitk_sumsq_kernel<4>, rg, dim3(1024), 0, ctx->stream, sbuf, Np * ncols, ncols, ss_part); break;
        case 8: hipLaunchKernelGGL(splitk_sumsq_kernel<8>, rg, dim3(1024), 0, ctx->stream, sbuf, Np * ncols, ncols, ss_part); break;
        default: hipLaunchKernelGGL(splitk_sumsq_kernel<16>, rg, dim3(1024), 0, ctx->stream, sbuf, Np * ncols, ncols, ss_part); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the post-processing of the context's model for a request
static FinishParams finish_params(const gpry_ctx* ctx, const SweepRequest& rq) {
    FinishParams fp;
    // (fp.C is the prior VARIANCE of a new point, C + w for a model with a white term: the finishes form var = fp.C - |V k*|^2
    // from it and the bound kernels of the pruned sweep their prior sigma, finish_sd(0, ..) -- acq_math.h)
    fp.C = ctx_prior_var(ctx); fp.y_mean = ctx->tf.y_mean; fp.y_std = ctx->tf.y_std;
    fp.clip_hi = ctx->tf.clip_hi; fp.zeta = rq.zeta; fp.baseline = rq.baseline; fp.sigma_n = rq.sigma_n;
    fp.want_std = rq.kind != SWEEP_PREDICT || rq.want_std; fp.want_acq = rq.kind != SWEEP_PREDICT;
    return fp;
}

// The chunk pipeline over the candidates resident in ctx->dXc: buffers, events, upload / overlap ordering, and per chunk
// "build, contract, finish" as the request's kind says (sweep.h: SweepRequest).
int run_sweep(gpry_ctx* ctx, int64_t M, const SweepRequest& rq) {
    const bool predict = rq.kind == SWEEP_PREDICT, stage_a = rq.kind == SWEEP_STAGE_A, y_given = rq.y_given;
    const int64_t Np = ctx->Np;
    const int nt = (int)(Np / 128);
    const int64_t chunk = sweep_chunk(ctx, M);
    // "sweep_overlap" = 1 (round 6): the cross-kernel panel of chunk c + 1 is built on the side stream while the main stream
    // contracts chunk c -- two panels and two sets of partial sums, one event per hand-over.  Same kernels on the same data:
    // same bits.  Only for sweeps of several chunks with the one-pass contraction.
    const bool overlap = ctx->opt_sweep_overlap && ctx->stream2 != nullptr && rq.kind == SWEEP_FULL && M > chunk;
    const int nbuf = overlap ? 2 : 1;
    if (stage_a) GPRY_TRY(dev_grow(ctx, &ctx->dub, &ctx->ub_cap, round_up(M, 1024)));
    else GPRY_TRY(dev_grow(ctx, &ctx->dKst, &ctx->kst_cap, nbuf * Np * chunk));
    // gpry_predict with a few hundred points: the panel comes from the small-batch kernel, which leaves
    // four mean partials per 128 training rows (kernel_build.hip: cross_build_small_kernel)
    const bool small_build = predict && M <= 512;
    const int nt_mean = small_build ? 4 * nt : nt;
    const int64_t part_stride = (int64_t)(nt_mean + nt) * chunk;
    GPRY_TRY(ensure_part(ctx, nbuf * part_stride));
    const FinishParams fp = finish_params(ctx, rq);
    ctx->sw_M = M;
    GPRY_TRY(choose_panel_form(ctx, small_build));
    const int form = ctx->panel_form;
    const bool no_panel = stage_a && y_given;
    if (panel_from_matrix_pipe(form) && !no_panel) GPRY_TRY(launch_cross_prepare(ctx));
    if (stage_a) ctx->prune.form = form;
    const MeanBound mb = mean_bound_setup(ctx, rq, fp, nt);
    unsigned long long* live_cnt = nullptr;
    if (stage_a) { ctx->prune.ybound = mb.on ? 1 : 0; ctx->prune.live_blocks = 0; ctx->prune.blocks = 0; ctx->prune.cert_blocks = 0; }
    if (mb.on) {
        if (!ctx->dsel) GPRY_TRY(dev_alloc(ctx, &ctx->dsel, gpry_ctx::DSEL_WORDS));
        live_cnt = ctx->dsel + gpry_ctx::DSEL_LIVE;
        HIP_TRY(ctx, hipMemsetAsync(live_cnt, 0, 16, ctx->stream));       // (DSEL_LIVE and DSEL_FALL)
        if (getenv("GPRY_HIP_DEBUG_PANEL"))
            fprintf(stderr, "gpry: bound pass: u in [%.6g, %.3g] skipped, D %.3g, gamma %.3g\n", mb.ubnd, mb.uhi, mb.D1, mb.g3 / 3.0);
    }
    // A fresh pool (gpry_sweep_logexp with a host array, option "sweep_upload"): the rows of chunk c go up on stream2 while
    // the main stream still works on chunk c - 1 -- 4.2 MB against 7.7 ms of kernels at N = 4096 -- and the main stream
    // waits for nothing but its own chunk (one event per chunk, never re-recorded within a call).  From pageable memory
    // hipMemcpyAsync returns when the rows are staged, so the host is one chunk ahead of the GPU, which is all it takes.
    const double* up_X = ctx->up_X;
    const double* up_y = ctx->up_y;
    const size_t nchunk = (size_t)((M + chunk - 1) / chunk);
    if (up_X || overlap) {
        while (ctx->ev_pool.size() < 3 * nchunk + 1) {
            hipEvent_t ev;
            HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ctx->ev_pool.push_back(ev);
        }
    }
    const hipStream_t main_stream = ctx->stream, side = ctx->stream2;
    // the launchers queue on ctx->stream: for the work of the side stream it is swapped for the duration of the call
    struct StreamSwap {
        gpry_ctx* c; hipStream_t keep;
        StreamSwap(gpry_ctx* ctx, hipStream_t st) : c(ctx), keep(ctx->stream) { c->stream = st; }
        ~StreamSwap() { c->stream = keep; }
    };
    // upload (and gates) of chunk ci on the side stream; `ev_up` = ev_pool[ci]
    auto upload_chunk = [&](size_t ci, bool gates_on_side) -> int {
        const int64_t m0 = (int64_t)ci * chunk, mc = (M - m0 < chunk) ? M - m0 : chunk;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dXc + m0 * ctx->d, up_X + m0 * ctx->d, sizeof(double) * mc * ctx->d,
                                    hipMemcpyHostToDevice, side));
        if (up_y) HIP_TRY(ctx, hipMemcpyAsync(ctx->dy_all + m0, up_y + m0, sizeof(double) * mc, hipMemcpyHostToDevice, side));
        if (gates_on_side && ctx->up_gates) {
            StreamSwap sw(ctx, side);
            StageScope s(ctx, "gates");
            GPRY_TRY(launch_gates(ctx, ctx->dXc + m0 * ctx->d, mc, ctx->dmask + m0));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[ci], side));
        return 0;
    };
    auto build_panel = [&](size_t ci, double* Kst, double* mean_part) -> int {
        const int64_t m0 = (int64_t)ci * chunk, mc = (M - m0 < chunk) ? M - m0 : chunk, mcp = round_up(mc, 128);
        StageScope s(ctx, stage_a ? "sweep_mean" : "cross_build");
        if (stage_a) Kst = nullptr;         // (the kernels store the mean partials only)
        if (y_given) mean_part = nullptr;   // (... or the panel only)
        if (mb.on) {                        // (bound partials, the sums of |terms| in the place of the sigma partials)
            // The blocks cross_build_mfma_kernel<.., BND> walks in this launch: grid.x workgroups of 4 waves, nt row chunks, and per
            // wave 8 steps of 16 rows x 2 blocks of 32 candidates.  sweep_impl derives the certified blocks from this count (all -
            // live - skipped by the FP64 test), so it has to follow the kernel's loop and launch_cross_mean_bound's grid.
            ctx->prune.blocks += (int64_t)((mcp + 255) / 256) * 4 * nt * 16;
            return launch_cross_mean_bound(ctx, ctx->dXc, m0, mcp, mean_part, mean_part + (int64_t)nt_mean * chunk, mb.ubnd, mb.uhi, live_cnt);
        }
        return build_sweep_panel(ctx, form, ctx->dXc, m0, mcp, Kst, mean_part);
    };
    if (overlap) {
        // the side stream starts behind what the main stream has queued so far (the scaled / centred training rows, the mask)
        hipEvent_t ev0 = ctx->ev_pool[3 * nchunk];
        HIP_TRY(ctx, hipEventRecord(ev0, main_stream));
        HIP_TRY(ctx, hipStreamWaitEvent(side, ev0, 0));
        if (up_X) GPRY_TRY(upload_chunk(0, true));
        { StreamSwap sw(ctx, side); GPRY_TRY(build_panel(0, ctx->dKst, ctx->dpart)); }
        HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[nchunk], side));
    }
    for (int64_t m0 = 0; m0 < M; m0 += chunk) {
        int64_t mc = (M - m0 < chunk) ? M - m0 : chunk;
        int64_t mcp = round_up(mc, 128);
        const size_t ci = (size_t)(m0 / chunk);
        const int buf = overlap ? (int)(ci & 1) : 0;
        double* Kst = ctx->dKst + (int64_t)buf * Np * chunk;
        double* mean_part = ctx->dpart + (int64_t)buf * part_stride;
        double* ss_part = mean_part + (int64_t)nt_mean * chunk;
        if (overlap) {
            // side stream: upload and panel of the NEXT chunk, into the buffers chunk ci - 1 has finished with
            if (ci + 1 < nchunk) {
                if (up_X) GPRY_TRY(upload_chunk(ci + 1, true));
                if (ci >= 1) HIP_TRY(ctx, hipStreamWaitEvent(side, ctx->ev_pool[2 * nchunk + ci - 1], 0));
                const int nb = (int)((ci + 1) & 1);
                { StreamSwap sw(ctx, side); GPRY_TRY(build_panel(ci + 1, ctx->dKst + (int64_t)nb * Np * chunk, ctx->dpart + (int64_t)nb * part_stride)); }
                HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[nchunk + ci + 1], side));
            }
            HIP_TRY(ctx, hipStreamWaitEvent(main_stream, ctx->ev_pool[nchunk + ci], 0));
        } else {
            if (up_X) {
                GPRY_TRY(upload_chunk(ci, false));
                HIP_TRY(ctx, hipStreamWaitEvent(main_stream, ctx->ev_pool[ci], 0));
                if (ctx->up_gates) {        // the SVM / trust-region verdicts of this chunk, on top of the caller's bits
                    StageScope s(ctx, "gates");
                    GPRY_TRY(launch_gates(ctx, ctx->dXc + m0 * ctx->d, mc, ctx->dmask + m0));
                }
            }
            if (!no_panel) GPRY_TRY(build_panel(ci, Kst, mean_part));
        }
        const uint8_t* mask = rq.have_mask ? ctx->dmask : nullptr;
        const dim3 fgrid((unsigned)((mc + 255) / 256)), fblock(256);
        if (stage_a) {      // nothing is contracted: y (or its bound), the bound of the acquisition, PRUNED_SIGMA
            StageScope s(ctx, no_panel ? "sweep_given_bound" : "sweep_mean");
            if (no_panel)
                hipLaunchKernelGGL(sweep_given_bound_kernel, fgrid, fblock, 0, ctx->stream,
                                   m0, mc, mask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all, ctx->dub, fp);
            else if (mb.on)
                hipLaunchKernelGGL(sweep_mean_bound_kernel, fgrid, fblock, 0, ctx->stream,
                                   mean_part, ss_part, nt_mean, mcp, m0, mc, mask,
                                   ctx->dy_all, ctx->dsig_all, ctx->dacq_all, ctx->dub, fp, mb.D1, mb.g3);
            else
                hipLaunchKernelGGL(sweep_mean_kernel, fgrid, fblock, 0, ctx->stream,
                                   mean_part, nt_mean, mcp, m0, mc, mask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all, ctx->dub, fp);
            HIP_TRY(ctx, hipGetLastError());
            continue;
        }
        const int nsplit = predict && fp.want_std && ctx->opt_predict_split && M <= chunk ? predict_nsplit(ctx, mcp) : 1;
        if (nsplit > 1) {
            StageScope s(ctx, "sweep_gemm_splitk");
            GPRY_TRY(contract_splitk(ctx, Kst, mcp, nsplit, ss_part));
        } else if (fp.want_std) {
            StageScope s(ctx, "sweep_gemm");
            GPRY_TRY(contract_sweep(ctx, Kst, mcp, ss_part));
        }
        {
            StageScope s(ctx, "sweep_finish");
            if (y_given)
                hipLaunchKernelGGL(sweep_given_finish_kernel, fgrid, fblock, 0, ctx->stream,
                                   ss_part, nt, mcp, m0, mc, mask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all, fp);
            else
                hipLaunchKernelGGL(sweep_finish_kernel, fgrid, fblock, 0, ctx->stream,
                                   mean_part, ss_part, nt_mean, nt, mcp, m0, mc, mask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all, fp);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (overlap) HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[2 * nchunk + ci], main_stream));
    }
    return 0;
}

int upload_candidates(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, bool upload_later) {
    GPRY_TRY(ensure_sweep_buffers(ctx, M));
    if (X) HIP_TRY(ctx, hipMemcpyAsync(ctx->dXc, X, sizeof(double) * M * ctx->d, hipMemcpyHostToDevice, ctx->stream));
    else if (upload_later) { }      // (the caller's rows reach dXc chunk by chunk inside run_sweep)
    else if (ctx->sw_M != M) return gpry_fail(ctx, -1, "X == NULL but no resident candidate set of size %lld", (long long)M);
    if (mask) HIP_TRY(ctx, hipMemcpyAsync(ctx->dmask, mask, (size_t)M, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

__global__ void count_nan_kernel(const double* __restrict__ a, int64_t n, unsigned long long* out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (; i < n; i += stride) c += (a[i] != a[i]) ? 1ull : 0ull;
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// THE COMPACT BATCHES of a pruned sweep (the rounds: sweep_topk.hip).  Bits: a candidate's panel column and mean partials depend on its coordinates alone (kernel_build.hip), and the one-pass
// contraction's per-tile partials of a column depend only on that column, the row tile and the k direction of the row tile,
// which is a function of the row tile and Np alone (sweep_gemm.hip) -- not of which other candidates share the launch or
// where the column falls in it.  The compact batches therefore give every candidate the bits of the full sweep.  (Split-K
// is never used here: it sums in another order.)

// the pool indices of every candidate not contracted yet (the completion)
__global__ void pruned_idx_kernel(const double* __restrict__ sig, int64_t M, int64_t* __restrict__ idx, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M && sig[i] == PRUNED_SIGMA) idx[atomicAdd(cnt, 1ull)] = i;
}

// Stage A's model, kept for the contraction rounds and the completion: V, alpha_, the training rows (raw and scaled for
// theta), theta, kernel, affine maps, centre.  NORA refits and refactorises between a lazy sweep and the next call, whose
// re-weighting fetches the arrays of the OLD model; these copies (one Np x Np copy, ~0.1 ms at Np = 4096) are what lets a
// pruned sweep be completed later with the model it was made with, as the full sweep's arrays would have been.
static int prune_snapshot(gpry_ctx* ctx) {
    GPRY_TRY(ensure_pred_xs(ctx));          // dXs scaled for the prediction factor's theta
    gpry_ctx::ModelSnap& m = ctx->snap;
    const int64_t Np = ctx->Np, N = ctx->N;
    GPRY_TRY(dev_grow(ctx, &m.dV, &m.v_cap, Np * Np));
    GPRY_TRY(dev_grow(ctx, &m.dalpha_, &m.a_cap, Np));
    GPRY_TRY(dev_grow(ctx, &m.dXs, &m.xs_cap, Np * ctx->dpad));
    GPRY_TRY(dev_grow(ctx, &m.dX, &m.x_cap, (N > 0 ? N : 1) * ctx->d));
    HIP_TRY(ctx, hipMemcpyAsync(m.dV, ctx->dV, sizeof(double) * Np * Np, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(m.dalpha_, ctx->dalpha_, sizeof(double) * Np, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(m.dXs, ctx->dXs, sizeof(double) * Np * ctx->dpad, hipMemcpyDeviceToDevice, ctx->stream));
    if (N > 0) HIP_TRY(ctx, hipMemcpyAsync(m.dX, ctx->dX, sizeof(double) * N * ctx->d, hipMemcpyDeviceToDevice, ctx->stream));
    m.N = N; m.Np = Np; m.d = ctx->d; m.dpad = ctx->dpad; m.kernel_id = ctx->kernel_id; m.white = ctx->white;
    memcpy(m.theta, ctx->theta, sizeof(m.theta));
    m.tf = ctx->tf;
    memcpy(m.xcenter, ctx->xcenter, sizeof(m.xcenter));
    m.xs_foreign = false;
    return 0;
}

// swaps the snapshot in for the duration of a contraction round / the completion (the launchers read the context)
struct SnapSwap {
    gpry_ctx* c;
    explicit SnapSwap(gpry_ctx* ctx) : c(ctx) { swap(); }
    ~SnapSwap() { swap(); }
    void swap() {
        gpry_ctx::ModelSnap& m = c->snap;
        std::swap(c->dV, m.dV); std::swap(c->dalpha_, m.dalpha_); std::swap(c->dXs, m.dXs); std::swap(c->dX, m.dX);
        std::swap(c->N, m.N); std::swap(c->Np, m.Np); std::swap(c->d, m.d); std::swap(c->dpad, m.dpad);
        std::swap(c->kernel_id, m.kernel_id); std::swap(c->white, m.white); std::swap(c->theta, m.theta); std::swap(c->tf, m.tf);
        std::swap(c->xcenter, m.xcenter); std::swap(c->xs_foreign, m.xs_foreign);
    }
};

// exact sigma / acq of the n candidates whose pool indices are in ctx->dgidx
int prune_eval(gpry_ctx* ctx, int64_t n) {
    SnapSwap model(ctx);                    // stage A's model, whatever happened to the context's since
    const int64_t Np = ctx->Np, M = ctx->sw_M;
    const int nt = (int)(Np / 128);
    const int64_t chunk = sweep_chunk(ctx, M);
    const int64_t np_max = round_up(n < chunk ? n : chunk, 128);
    GPRY_TRY(dev_grow(ctx, &ctx->dKst, &ctx->kst_cap, Np * np_max));
    // (after the bound pass the batch's mean partials as well, behind its sigma partials: y of the full sweep, bit for bit --
    // the panel kernels give a candidate's mean partials from its own coordinates alone)
    const bool want_y = ctx->prune.ybound != 0;
    GPRY_TRY(ensure_part(ctx, (int64_t)nt * np_max * (want_y ? 2 : 1)));
    // (in doubles, not rows: a later model may have more dimensions than the one the buffer was made for)
    GPRY_TRY(dev_grow(ctx, &ctx->dXg, &ctx->xg_cap, round_up(np_max, 256) * ctx->d));
    const int form = ctx->prune.form;       // the panel form of stage A (a gpry_predict in between may have built another)
    if (panel_from_matrix_pipe(form)) GPRY_TRY(launch_cross_prepare(ctx));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nc = (n - i0 < chunk) ? n - i0 : chunk, ncp = round_up(nc, 128), npad = round_up(ncp, 256);
        const int64_t* gidx = ctx->dgidx + i0;
        {
            StageScope s(ctx, "sweep_compact");
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((npad * ctx->d + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->dXc, ctx->d, gidx, nc, npad, ctx->dXg);
            HIP_TRY(ctx, hipGetLastError());
            // (the builders read rows below min(sw_M, round_up(ncp, 256)) = npad at most: dXg holds npad rows)
            double* mean_part = want_y ? ctx->dpart + (int64_t)nt * ncp : nullptr;
            GPRY_TRY(build_sweep_panel(ctx, form, ctx->dXg, 0, ncp, ctx->dKst, mean_part));
        }
        StageScope s(ctx, "sweep_prune_gemm");
        GPRY_TRY(contract_sweep(ctx, ctx->dKst, ncp, ctx->dpart));
        hipLaunchKernelGGL(sweep_scatter_finish_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, ctx->stream,
                           ctx->dpart, nt, ncp, gidx, nc, ctx->prune.have_mask ? ctx->dmask : nullptr, ctx->dy_all,
                           ctx->dsig_all, ctx->dacq_all, ctx->prune.fp, want_y ? ctx->dpart + (int64_t)nt * ncp : nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// the rest of the pool, contracted as the full sweep would have contracted it (stage A's model, same kernels, same bits):
// afterwards the resident arrays are the full sweep's
int prune_complete(gpry_ctx* ctx) {
    const int64_t M = ctx->sw_M;
    GPRY_TRY(dev_grow(ctx, &ctx->dgidx, &ctx->gidx_cap, round_up(M, 1024)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dsel + gpry_ctx::DSEL_GIDX, 0, 8, ctx->stream));
    hipLaunchKernelGGL(pruned_idx_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dsig_all, M, ctx->dgidx, ctx->dsel + gpry_ctx::DSEL_GIDX);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, ctx->dsel + gpry_ctx::DSEL_GIDX, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n > 0) GPRY_TRY(prune_eval(ctx, (int64_t)n));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->prune.evaluated_total += (int64_t)n;
    ctx->sw_pruned = 0;
    ctx->prune.completed = 1;
    return 0;
}

// The tail of a sweep entry point: the NaNs of nan_src counted into *nn (nan_src NULL: not counted), the live blocks of the
// bound pass and the blocks only its FP64 test skipped into live[0] and live[1] (NULL: not fetched), the arrays the caller wants copied out, one synchronisation.
static int sweep_copy_out(gpry_ctx* ctx, int64_t M, const double* nan_src, unsigned long long* nn, unsigned long long* live,
                          double* y_all, double* sigma_all, double* acq_all) {
    if (nan_src) {
        if (!ctx->dsel) GPRY_TRY(dev_alloc(ctx, &ctx->dsel, gpry_ctx::DSEL_WORDS));
        unsigned long long* dnan = ctx->dsel + gpry_ctx::DSEL_NAN;
        HIP_TRY(ctx, hipMemsetAsync(dnan, 0, 8, ctx->stream));
        hipLaunchKernelGGL(count_nan_kernel, dim3(1024), dim3(256), 0, ctx->stream, nan_src, M, dnan);
        HIP_TRY(ctx, hipMemcpyAsync(nn, dnan, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (live) HIP_TRY(ctx, hipMemcpyAsync(live, ctx->dsel + gpry_ctx::DSEL_LIVE, 16, hipMemcpyDeviceToHost, ctx->stream));
    if (y_all) HIP_TRY(ctx, hipMemcpyAsync(y_all, ctx->dy_all, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->stream));
    if (sigma_all) HIP_TRY(ctx, hipMemcpyAsync(sigma_all, ctx->dsig_all, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->stream));
    if (acq_all) HIP_TRY(ctx, hipMemcpyAsync(acq_all, ctx->dacq_all, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// gpry_sweep_logexp (y_given NULL) and the sigma-only case of gpry_sweep_logexp_given (y_given: the caller's M values, which go
// up with the pool and take the place of the posterior mean)
static int sweep_impl(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, const double* y_given, double zeta,
                      double baseline, double sigma_n, double* y_all, double* sigma_all, double* acq_all, int64_t* n_nan) {
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M <= 0) return gpry_fail(ctx, -1, "sweep: M must be > 0");
    // option "sweep_prune" and no arrays wanted (NORA's lazy path): stage A of the pruned sweep -- y and a bound of every
    // candidate's acquisition, nothing contracted yet; gpry_sweep_topk contracts what can reach the shortlist
    const bool prune = ctx->opt_sweep_prune && !y_all && !sigma_all && !acq_all;
    ctx->sw_pruned = 0;
    // a pool that comes from the host goes up chunk by chunk underneath the sweep itself (run_sweep); "sweep_upload" = 0:
    // in one piece in front of it (the comparator)
    const bool piped = X != nullptr && ctx->opt_sweep_upload && ctx->stream2 != nullptr;
    GPRY_TRY(upload_candidates(ctx, piped ? nullptr : X, M, mask, piped));
    SweepRequest rq;
    rq.kind = prune ? SWEEP_STAGE_A : SWEEP_FULL; rq.have_mask = mask != nullptr; rq.y_given = y_given != nullptr;
    rq.zeta = zeta; rq.baseline = baseline; rq.sigma_n = sigma_n;
    if (ctx->gates_on) {
        // the SVM / trust-region verdicts are computed here, on top of the caller's bits
        if (!rq.have_mask) HIP_TRY(ctx, hipMemsetAsync(ctx->dmask, 0, (size_t)M, ctx->stream));
        if (!piped) {
            StageScope s(ctx, "gates");
            GPRY_TRY(launch_gates(ctx, ctx->dXc, M, ctx->dmask));
        }
        rq.have_mask = true;
    }
    struct UploadScope {        // (cleared on every way out: a later sweep of the resident pool must not upload again)
        gpry_ctx* c; bool done = false;
        ~UploadScope() {
            c->up_X = nullptr; c->up_y = nullptr; c->up_gates = 0;
            // a sweep that did not complete leaves no resident pool behind: with the chunked upload part of dXc would be
            // stale, and a later call with X == NULL must not pass the size check; the side stream is drained as well
            if (!done) { c->sw_M = 0; if (c->stream2) (void)hipStreamSynchronize(c->stream2); (void)hipStreamSynchronize(c->stream); }
        }
    } upload_scope{ctx};
    if (piped) { ctx->up_X = X; ctx->up_gates = ctx->gates_on ? 1 : 0; }
    if (y_given) {
        if (piped) ctx->up_y = y_given;     // (chunk by chunk beside the rows)
        else HIP_TRY(ctx, hipMemcpyAsync(ctx->dy_all, y_given, sizeof(double) * M, hipMemcpyHostToDevice, ctx->stream));
    }
    GPRY_TRY(run_sweep(ctx, M, rq));
    // (pruned: the bound is NaN exactly where y is.  The exact acquisition of a candidate with a finite y is not NaN either: a
    // NaN per-tile sum needs a NaN in V or in the candidate's panel column, and either one reaches y -- alpha_ = V^T V y
    // picks up every entry of V in alpha_[0], and a NaN panel entry enters the mean partial through fma(alpha_j, k, .), NaN
    // for any alpha_j.  The rest of the finish keeps var in [0, C]: the acquisition is finite or -inf.)
    unsigned long long nn = 0, live[2] = {0, 0};
    GPRY_TRY(sweep_copy_out(ctx, M, prune ? ctx->dub : ctx->dacq_all, &nn, prune && ctx->prune.ybound ? live : nullptr,
                            y_all, sigma_all, acq_all));
    upload_scope.done = true;
    if (n_nan) *n_nan = (int64_t)nn;
    if (prune) {
        const int form = ctx->prune.form, ybound = ctx->prune.ybound;
        const int64_t blocks = ctx->prune.blocks;
        ctx->prune = gpry_ctx::PruneState();
        ctx->prune.form = form;
        ctx->prune.ybound = ybound;
        ctx->prune.live_blocks = ybound ? (int64_t)live[0] : 0;
        // (every block is certified by the screen, skipped by the FP64 test or live)
        ctx->prune.cert_blocks = ybound && ctx->opt_sweep_screen ? blocks - (int64_t)live[0] - (int64_t)live[1] : 0;
        ctx->prune.blocks = ybound ? blocks : 0;
        ctx->prune.have_mask = rq.have_mask ? 1 : 0;
        ctx->prune.fp = finish_params(ctx, rq);
        GPRY_TRY(prune_snapshot(ctx));
        ctx->sw_pruned = 1;
    }
    return 0;
}

extern "C" {

int gpry_sweep_info(gpry_ctx* ctx, int* panel_form, double* est) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_info: ctx is NULL");
    if (panel_form) *panel_form = ctx->panel_form;
    if (est) for (int k = 0; k < 4; k++) est[k] = ctx->panel_est[k];
    return 0;
}

int gpry_sweep_fetch(gpry_ctx* ctx, int64_t M, double* y_all, double* sigma_all, double* acq_all) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_fetch: ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M <= 0 || M != ctx->sw_M) return gpry_fail(ctx, -1, "sweep_fetch: the resident sweep has %lld candidates, not %lld",
                                                  (long long)ctx->sw_M, (long long)M);
    // (test hook "panel_debug" & 256: the arrays as they stand -- bounds where nothing was contracted -- and no completion)
    if (ctx->sw_pruned && !(ctx->opt_panel_debug & 256)) GPRY_TRY(prune_complete(ctx));      // the arrays of the full sweep, bit for bit
    return sweep_copy_out(ctx, M, nullptr, nullptr, nullptr, y_all, sigma_all, acq_all);
}

int gpry_sweep_logexp(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, double zeta,
                      double baseline, double sigma_n, double* y_all, double* sigma_all, double* acq_all,
                      int64_t* n_nan) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_logexp: ctx is NULL");
    return sweep_impl(ctx, X, M, mask, nullptr, zeta, baseline, sigma_n, y_all, sigma_all, acq_all, n_nan);
}

int gpry_sweep_logexp_given(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, const double* y_given,
                            const double* sigma_given, double zeta, double baseline, double sigma_n, double* y_all,
                            double* sigma_all, double* acq_all, int64_t* n_nan) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_logexp_given: ctx is NULL");
    if (!y_given) return gpry_fail(ctx, -1, "sweep_logexp_given: y_given must not be NULL");
    if (!sigma_given)
        return sweep_impl(ctx, X, M, mask, y_given, zeta, baseline, sigma_n, y_all, sigma_all, acq_all, n_nan);
    // both given: acq = LogExp.f(y, sigma_y) and nothing else -- no panel, no gates, no mask (the mask argument is ignored).
    // No factor is read, so none is required; the pool rows are still taken (X != NULL) so that the resident pool stays
    // the one the arrays belong to, which needs the row width of gpry_set_train.
    GPRY_TRY(serve_stop(ctx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M <= 0) return gpry_fail(ctx, -1, "sweep: M must be > 0");
    if (X && ctx->d <= 0) return gpry_fail(ctx, -1, "sweep_logexp_given: set_train before a pool of rows");
    ctx->sw_pruned = 0;
    GPRY_TRY(upload_candidates(ctx, X, M, nullptr));
    ctx->sw_M = 0;                          // (until the call completes: no resident pool behind a failed one)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dy_all, y_given, sizeof(double) * M, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dsig_all, sigma_given, sizeof(double) * M, hipMemcpyHostToDevice, ctx->stream));
    {
        StageScope s(ctx, "sweep_finish");
        GPRY_TRY(launch_logexp(ctx, ctx->dy_all, ctx->dsig_all, M, zeta, baseline, sigma_n, ctx->dacq_all));
    }
    unsigned long long nn = 0;
    GPRY_TRY(sweep_copy_out(ctx, M, ctx->dacq_all, &nn, nullptr, y_all, sigma_all, acq_all));
    ctx->sw_M = M;
    if (n_nan) *n_nan = (int64_t)nn;
    return 0;
}

}  // extern "C"
