// Joint posterior covariance of the surrogate at a batch of points, and joint draws from it: the kernels behind
// gpry_predict_cov and gpry_sample_joint.  What is done with the draws (the spread of the posterior mean, of the
// covariance and of log Z over realisations of the surrogate) is host-side, in gpry_amd/mc.py: surrogate_spread.
//
// The reference returns no covariance ("cannot return the full covariance matrix ... to save on some complexity",
// gpry/gpr.py:1062-1067); the closed form is sklearn's (_gpr.py:430-438): with U = V K*^T, V = L^-1,
//   Sigma = y_std^2 (K(X*, X*) - U^T U).
// The chain of a call: the cross-kernel panel K*^T (Np x mp, the existing builders, the small one up to 512 padded
// points), U by the triangular GEMM, the Gram U^T U by the same engine (lower tiles only) into the m-padded square,
// then joint_finish_kernel -- a pass of its own over the lower triangle -- which takes the prior entry from the scaled
// coordinates (corr_r2_fast, the panel's own routine), subtracts the Gram entry, scales by y_std^2, clears the rows and
// columns of classifier-rejected points and writes the entry and its mirror image.  Both GEMMs split their k-ranges by
// the model size alone, so an entry is one fixed chain of multiply-adds over the training rows: Sigma_ab depends on the
// model and the two points, not on m, on their places in the batch or on the context.
//
// A draw is Y_s = mu + L_c z_s, L_c the lower Cholesky factor (the panel chain, potrf_lower_overlap, on the padded
// square) of Sigma + eps C y_std^2 I, with the identity on the diagonal of the padding and of rejected rows.
// joint_product_kernel forms Y = mu + Z L_c^T with v_mfma_f64_16x16x4: a workgroup owns 32 draws x 128 points, walks
// the columns j of L_c sixteen at a time from 0 to the end of its own diagonal tile (the tiles above the diagonal are
// never visited, the entries above it inside the diagonal tile are read as zeros), and makes the 32 x 16 normal variates
// of a step in LDS itself -- one Philox counter (phase NS_PHASE_JOINT, draw s, pair j / 2) and one Box-Muller pair per
// thread -- so z_sj depends on (seed, s, j) alone and Y_si is one chain over j ascending: the same bits whatever S.
#include "ns_common.h"
#include <vector>

#define JOINT_MAX_M 4096
#define JOINT_MAX_S 65536
#define JT_S 32           // draws per workgroup of the product
#define JT_I 128          // points per workgroup
#define JT_K 16           // columns of L_c per step
#define JT_LD 18          // row stride (doubles) of both LDS images: the fragment reads are bank-conflict free (gemm_f64.hip: SKC)

// rows of the batch mapped to the kernel's coordinates, row-major with dpad columns (zeros beyond d and beyond m)
__global__ __launch_bounds__(256) void joint_scale_kernel(const double* __restrict__ X, int64_t m, int64_t mp, int d, int dpad,
                                                          int has_aff, AffParams ap, double* __restrict__ Xs) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= mp * dpad) return;
    const int64_t i = idx / dpad;
    const int k = (int)(idx - i * dpad);
    double v = 0.0;
    if (k < d && i < m) {
        v = X[i * d + k];
        if (has_aff) v = (v - ap.lo[k]) / ap.span[k];
        v = v / ap.ls[k];
    }
    Xs[idx] = v;
}

// mu_i = (sum of the panel's mean partials, in their order) y_std + y_mean: the unclipped, ungated mean in units of y
__global__ __launch_bounds__(256) void joint_mu_kernel(const double* __restrict__ mpart, int ntm, int64_t mp, int64_t m,
                                                       double y_std, double y_mean, double* __restrict__ mu) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mp) return;
    double s = 0.0;
    if (i < m)
        for (int t = 0; t < ntm; t++) s += mpart[(int64_t)t * mp + i];
    mu[i] = i < m ? ns_rn(s * y_std) + y_mean : 0.0;
}

// Sig holds the Gram U^T U in its lower tiles on entry; on exit the whole mp x mp square holds Sigma (zeros in the padding)
template <int KID>
__global__ __launch_bounds__(256) void joint_finish_kernel(double* __restrict__ Sig, int64_t mp, int64_t m,
                                                           const double* __restrict__ Xs, int dpad, double C, double ys2,
                                                           const uint8_t* __restrict__ mask) {
    if (blockIdx.x > blockIdx.y) return;
    const int64_t a = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4), b = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    if (b > a || a >= mp) return;
    double v = 0.0;
    if (a < m && !((mask[a] | mask[b]) & GPRY_MASK_CLASSIFIED_INF)) {        // (b <= a < m)
        double r2 = 0.0;
        for (int k = 0; k < dpad; k++) {
            const double df = Xs[a * dpad + k] - Xs[b * dpad + k];
            r2 = fma(df, df, r2);
        }
        v = (C * corr_r2_fast<KID>(r2) - Sig[a * mp + b]) * ys2;
    }
    Sig[a * mp + b] = v;
    Sig[b * mp + a] = v;
}

// A = Sigma + eps on the diagonal of the rows that take part, 1 on the diagonal of the others (padding, rejected rows)
__global__ __launch_bounds__(256) void joint_shift_kernel(const double* __restrict__ Sig, double* __restrict__ A, int64_t mp,
                                                          int64_t m, double eps_abs, const uint8_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= mp * mp) return;
    const int64_t a = idx / mp, b = idx - a * mp;
    double v = Sig[idx];
    if (a == b) v = (a < m && !(mask[a] & GPRY_MASK_CLASSIFIED_INF)) ? v + eps_abs : 1.0;
    A[idx] = v;
}

// the diagonals of Sigma and of the factor, side by side (out: 2 m doubles)
__global__ __launch_bounds__(256) void joint_diag_kernel(const double* __restrict__ Sig, const double* __restrict__ Lc, int64_t mp,
                                                         int64_t m, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    out[i] = Sig[i * (mp + 1)];
    out[m + i] = Lc[i * (mp + 1)];
}

// the strict upper triangle of the factored square is what potrf left there: cleared for a caller who asks for L_c
__global__ __launch_bounds__(256) void joint_clear_upper_kernel(double* __restrict__ A, int64_t mp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= mp * mp) return;
    const int64_t a = idx / mp, b = idx - a * mp;
    if (b > a) A[idx] = 0.0;
}

// Y (S x m) = mu + Z L_c^T.  grid: (mp / JT_I point tiles, ceil(S / JT_S) draw tiles); 256 threads = 4 waves, wave
// (ws = wave >> 1, wc = wave & 1) owns draws 16 ws .. + 15 and points 64 wc .. + 63 of the tile as four accumulators.
// Operand and accumulator layout of the MFMA: chol16.h.
__global__ __launch_bounds__(256) void joint_product_kernel(const double* __restrict__ Lc, int64_t mp, int64_t m, int64_t S,
                                                            unsigned long long seed, const double* __restrict__ mu,
                                                            const uint8_t* __restrict__ mask, double* __restrict__ Y,
                                                            double* __restrict__ Zout) {
    __shared__ double sZ[JT_S * JT_LD];
    __shared__ double sL[JT_I * JT_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ws = wave >> 1, wc = wave & 1, r = lane & 15, gq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * JT_I, s0 = (int64_t)blockIdx.y * JT_S;
    const int64_t jend = i0 + JT_I;                   // (<= mp: the columns right of the tile's diagonal block are zero)
    v4d acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) acc[n] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int zs = t >> 3, zp = t & 7;                // this thread's variates of a step: draw s0 + zs, columns j0 + 2 zp, + 1
    const int lrow = t >> 1, lcol = (t & 1) * 8;      // ... and its piece of the L_c image: row i0 + lrow, 8 columns
    for (int64_t j0 = 0; j0 < jend; j0 += JT_K) {
        {
            const NsU2 u = ns_philox(seed, NS_PHASE_JOINT, 0u, (unsigned)(s0 + zs), (unsigned)((j0 >> 1) + zp), 0u);
            ns_box_muller(sZ + zs * JT_LD, zp, JT_K, u);
            const int64_t i = i0 + lrow;
            const double* src = Lc + i * mp + j0 + lcol;
#pragma unroll
            for (int e = 0; e < 8; e++) sL[lrow * JT_LD + lcol + e] = (j0 + lcol + e <= i) ? src[e] : 0.0;
        }
        __syncthreads();
        if (Zout && j0 >= i0 && s0 + zs < S) {        // the tile whose diagonal block these columns belong to hands them out
            const int64_t j = j0 + 2 * zp;
            if (j < m) Zout[(s0 + zs) * m + j] = sZ[zs * JT_LD + 2 * zp];
            if (j + 1 < m) Zout[(s0 + zs) * m + j + 1] = sZ[zs * JT_LD + 2 * zp + 1];
        }
#pragma unroll
        for (int kk = 0; kk < JT_K / 4; kk++) {
            const double a = sZ[(ws * 16 + r) * JT_LD + kk * 4 + gq];
#pragma unroll
            for (int n = 0; n < 4; n++) {
                const double b = sL[(wc * 64 + n * 16 + r) * JT_LD + kk * 4 + gq];
                acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const int64_t i = i0 + wc * 64 + n * 16 + r;
        if (i >= m) continue;
        const bool dead = mask[i] & GPRY_MASK_CLASSIFIED_INF;
        const double mui = mu[i];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t s = s0 + ws * 16 + gq + 4 * q;
            if (s < S) Y[s * m + i] = dead ? -INFINITY : mui + acc[n][q];
        }
    }
}

namespace {

struct JointWork {
    CallScratch cs;                  // held from joint_cov to the end of the entry point that owns this
    JointWork(gpry_ctx* ctx, const char* who) : cs(ctx, who) {}
    int64_t m = 0, mp = 0;
    int ntm = 0;
    double *X = nullptr, *Xs = nullptr, *Kst = nullptr, *U = nullptr, *mpart = nullptr, *mu = nullptr, *Sig = nullptr,
           *Lc = nullptr, *Y = nullptr, *Z = nullptr;
    uint8_t* mask = nullptr;
    std::vector<uint8_t> hmask;      // the caller's mask with the device gates ORed in
};

// split-K factor of the two products: a function of the model size alone (see gpry_kb_register)
int joint_ksplit(int64_t Np) {
    int ns = 1;
    while (ns < 8 && Np / (ns * 2) >= 256) ns *= 2;
    return ns;
}

int joint_check(gpry_ctx* ctx, const char* who, const double* X, int64_t m) {
    if (!X) return gpry_fail(ctx, -1, "%s: X is NULL", who);
    if (m < 1 || m > JOINT_MAX_M) return gpry_fail(ctx, -1, "%s: m = %lld, need 1 <= m <= %d", who, (long long)m, JOINT_MAX_M);
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "%s: d = %d > %d", who, ctx->d, GPRY_MAX_DIM);
    return check_points_finite(ctx, who, X, m);
}

// everything up to Sigma and mu on the device (queued on ctx->stream; the merged mask is on the host when this returns)
int joint_cov(gpry_ctx* ctx, const double* X, int64_t m, const uint8_t* mask, int64_t S, bool want_z, JointWork* w) {
    hipStream_t st = ctx->stream;
    const int64_t Np = ctx->Np, mp = round_up(m, 128);
    const int d = ctx->d, dpad = ctx->dpad, nt = (int)(Np / 128);
    const bool small_build = mp <= 512;
    w->m = m; w->mp = mp; w->ntm = small_build ? 4 * nt : nt;
    // The call scratch, in this order.  Nothing below claims it again (the panel builders, the GEMM engine and, in
    // gpry_sample_joint, potrf_lower_overlap take their buffers from the caller or from dsplit), and every launch and copy
    // of the two entry points is on ctx->stream, which they drain (ns_end) before the claim ends.
    CallScratch& cs = w->cs;
    const auto rX = cs.take<double>(m * d), rXs = cs.take<double>(mp * dpad), rKst = cs.take<double>(Np * mp),
               rU = cs.take<double>(Np * mp), rmpart = cs.take<double>((int64_t)w->ntm * mp), rmu = cs.take<double>(mp),
               rSig = cs.take<double>(mp * mp), rLc = cs.take<double>(S > 0 ? mp * mp : 0), rY = cs.take<double>(S * m),
               rZ = cs.take<double>(want_z ? S * m : 0);
    const auto rmask = cs.take<uint8_t>(mp);
    GPRY_TRY(cs.claim());
    w->X = cs.at(rX); w->Xs = cs.at(rXs); w->Kst = cs.at(rKst); w->U = cs.at(rU); w->mpart = cs.at(rmpart); w->mu = cs.at(rmu);
    w->Sig = cs.at(rSig); w->Lc = cs.at(rLc); w->Y = cs.at(rY); w->Z = cs.at(rZ); w->mask = cs.at(rmask);
    w->hmask.assign((size_t)mp, 0);
    if (mask) memcpy(w->hmask.data(), mask, (size_t)m);
    HIP_TRY(ctx, hipMemcpyAsync(w->X, X, sizeof(double) * m * d, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(w->mask, w->hmask.data(), (size_t)mp, hipMemcpyHostToDevice, st));
    if (ctx->gates_on && ctx->opt_predict_gates) {
        GPRY_TRY(launch_gates(ctx, w->X, m, w->mask));
        HIP_TRY(ctx, hipMemcpyAsync(w->hmask.data(), w->mask, (size_t)m, hipMemcpyDeviceToHost, st));
    }
    const int64_t saveM = ctx->sw_M; ctx->sw_M = m;
    const int rc = small_build ? launch_cross_build_small(ctx, w->X, 0, mp, mp, w->Kst, w->mpart, 1)
                               : launch_cross_build(ctx, w->X, 0, mp, mp, w->Kst, w->mpart, 1);
    ctx->sw_M = saveM;
    if (rc) return rc;
    const KernParams kp = make_kp(ctx);
    const AffParams ap = make_ap(ctx, kp.has_aff);
    hipLaunchKernelGGL(joint_scale_kernel, dim3((unsigned)((mp * dpad + 255) / 256)), dim3(256), 0, st, w->X, m, mp, d, dpad,
                       kp.has_aff, ap, w->Xs);
    hipLaunchKernelGGL(joint_mu_kernel, dim3((unsigned)(mp / 256 + 1)), dim3(256), 0, st, w->mpart, w->ntm, mp, m,
                       ctx->tf.y_std, ctx->tf.y_mean, w->mu);
    const int ns = joint_ksplit(Np);
    {   // U = V K*^T
        GemmArgs g = {};
        g.A = ctx->dV; g.lda = Np; g.B = w->Kst; g.ldb = mp; g.C = w->U; g.ldc = mp;
        g.M = (int)Np; g.N = (int)mp; g.K = (int)Np; g.kmode = KM_A_LOWER; g.tile_map = TM_ROWMAJOR;
        if (ns > 1) { GPRY_TRY(gemm_split_scratch(ctx, ns, Np * mp, &g.split_buf)); g.nsplit = ns; g.split_stride = Np * mp; }
        GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
    }
    {   // the Gram U^T U, lower tiles
        GemmArgs g = {};
        g.A = w->U; g.lda = mp; g.B = w->U; g.ldb = mp; g.C = w->Sig; g.ldc = mp;
        g.M = (int)mp; g.N = (int)mp; g.K = (int)Np; g.kmode = KM_FULL; g.lower_only = 1; g.tile_map = TM_ROWMAJOR;
        if (ns > 1) { GPRY_TRY(gemm_split_scratch(ctx, ns, mp * mp, &g.split_buf)); g.nsplit = ns; g.split_stride = mp * mp; }
        GPRY_TRY(gemm_f64_launch(ctx, g, true, false, EPI_STORE));
    }
    const unsigned nb = (unsigned)(mp / 16);
#define JF(KID) hipLaunchKernelGGL((joint_finish_kernel<KID>), dim3(nb, nb), dim3(256), 0, st, w->Sig, mp, m, w->Xs, dpad, \
                                   kp.C, ctx->tf.y_std * ctx->tf.y_std, w->mask)
    DISPATCH_KID(ctx->kernel_id, JF)
#undef JF
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the finalised mean of gpry_predict from mu: the clip, then the merged mask
void joint_mean(const gpry_ctx* ctx, const JointWork& w, const double* hmu, double* mean) {
    for (int64_t i = 0; i < w.m; i++) {
        double y = fmin(hmu[i], ctx->tf.clip_hi);
        if (w.hmask[(size_t)i]) y = -INFINITY;
        mean[i] = y;
    }
}

// the panel chain names a failing column no further than the training set's size: lend it the batch's for the call
struct RealSizeGuard {
    gpry_ctx* c; int64_t saved;
    RealSizeGuard(gpry_ctx* ctx, int64_t n) : c(ctx), saved(ctx->N) { c->N = n; }
    ~RealSizeGuard() { c->N = saved; }
};

}  // namespace

extern "C" {

int gpry_predict_cov(gpry_ctx* ctx, const double* X, int64_t m, const uint8_t* mask, double* mean, double* cov,
                     double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_cov: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    GPRY_TRY(refuse_white(ctx, "gpry_predict_cov"));
    if (!cov) return gpry_fail(ctx, -1, "gpry_predict_cov: cov is NULL");
    GPRY_TRY(joint_check(ctx, "gpry_predict_cov", X, m));
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    JointWork w(ctx, "gpry_predict_cov");
    std::vector<double> hmu;
    {
        StageScope scope(ctx, "predict_cov");
        GPRY_TRY(joint_cov(ctx, X, m, mask, 0, false, &w));
        HIP_TRY(ctx, hipMemcpy2DAsync(cov, sizeof(double) * m, w.Sig, sizeof(double) * w.mp, sizeof(double) * m, m,
                                      hipMemcpyDeviceToHost, ctx->stream));
        if (mean) {
            hmu.resize((size_t)m);
            HIP_TRY(ctx, hipMemcpyAsync(hmu.data(), w.mu, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    if (mean) joint_mean(ctx, w, hmu.data(), mean);
    return 0;
}

int gpry_sample_joint(gpry_ctx* ctx, const double* X, int64_t m, const uint8_t* mask, int64_t S, unsigned long long seed,
                      double jitter, double* mean, double* Y, double* Z_out, double* Lc_out, int* info,
                      double* jitter_used, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sample_joint: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    GPRY_TRY(refuse_white(ctx, "gpry_sample_joint"));
    if (!Y) return gpry_fail(ctx, -1, "gpry_sample_joint: Y is NULL");
    if (S < 1 || S > JOINT_MAX_S) return gpry_fail(ctx, -1, "gpry_sample_joint: S = %lld, need 1 <= S <= %d", (long long)S, JOINT_MAX_S);
    if (jitter != jitter || jitter == INFINITY) return gpry_fail(ctx, -1, "gpry_sample_joint: jitter = %g", jitter);
    GPRY_TRY(joint_check(ctx, "gpry_sample_joint", X, m));
    if (info) *info = 0;
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    JointWork w(ctx, "gpry_sample_joint");
    hipStream_t st = ctx->stream;
    const double unit = exp(ctx->theta[0]) * ctx->tf.y_std * ctx->tf.y_std;       // eps is in units of C y_std^2
    double eps = jitter < 0.0 ? 1e-10 : jitter;
    std::vector<double> hmu, hd((size_t)(2 * m));
    {
        StageScope scope(ctx, "sample_joint");
        GPRY_TRY(joint_cov(ctx, X, m, mask, S, Z_out != nullptr, &w));
        const int64_t mp = w.mp;
        const unsigned nbq = (unsigned)((mp * mp + 255) / 256);
        for (;;) {
            hipLaunchKernelGGL(joint_shift_kernel, dim3(nbq), dim3(256), 0, st, w.Sig, w.Lc, mp, m, eps * unit, w.mask);
            int hinfo[4] = {0, 0, 0, 0};
            {
                RealSizeGuard real(ctx, m);
                GPRY_TRY(potrf_lower_overlap(ctx, w.Lc, mp));
            }
            HIP_TRY(ctx, hipMemcpyAsync(hinfo, ctx->dinfo, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
            // the diagonals of Sigma and of L_c: a pivot within the factorisation's own rounding of zero is no pivot
            // (gathered into U, which is dead behind the Gram: Np mp >= 2 m doubles)
            hipLaunchKernelGGL(joint_diag_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, w.Sig, w.Lc, mp, m, w.U);
            HIP_TRY(ctx, hipMemcpyAsync(hd.data(), w.U, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if ((hinfo[3] & 0xFF00) == 0x5A00)
                return gpry_fail(ctx, -2, "gpry_sample_joint: Cholesky panel step timed out (wait %d)", hinfo[3] & 0xFF);
            int64_t bad = hinfo[0] != 0 ? hinfo[0] : hinfo[1];                   // 1-based failing column
            double dmax = 0.0;
            for (int64_t i = 0; i < m; i++) dmax = fmax(dmax, hd[(size_t)i] + eps * unit);
            const double tol = 8.0 * (double)(m + 1) * 0x1.0p-53 * dmax;
            for (int64_t i = 0; bad == 0 && i < m; i++) {
                const double l = hd[(size_t)(m + i)];
                if (!(l * l > tol)) bad = i + 1;
            }
            if (bad == 0) break;
            const double next = eps == 0.0 ? 1e-14 : eps * 100.0;
            if (next > 1e-4) {
                if (info) *info = (int)bad;
                if (jitter_used) *jitter_used = eps;
                return gpry_fail(ctx, -3, "gpry_sample_joint: pivot %lld of Sigma + %g C y_std^2 I is not positive; the jitter "
                                          "ladder ends at 1e-4", (long long)bad, eps);
            }
            eps = next;
        }
        const dim3 grid((unsigned)(mp / JT_I), (unsigned)((S + JT_S - 1) / JT_S));
        hipLaunchKernelGGL(joint_product_kernel, grid, dim3(256), 0, st, w.Lc, mp, m, S, seed, w.mu, w.mask, w.Y, w.Z);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(Y, w.Y, sizeof(double) * S * m, hipMemcpyDeviceToHost, st));
        if (Z_out) HIP_TRY(ctx, hipMemcpyAsync(Z_out, w.Z, sizeof(double) * S * m, hipMemcpyDeviceToHost, st));
        if (Lc_out) {
            hipLaunchKernelGGL(joint_clear_upper_kernel, dim3(nbq), dim3(256), 0, st, w.Lc, mp);
            HIP_TRY(ctx, hipMemcpy2DAsync(Lc_out, sizeof(double) * m, w.Lc, sizeof(double) * mp, sizeof(double) * m, m,
                                          hipMemcpyDeviceToHost, st));
        }
        if (mean) {
            hmu.resize((size_t)m);
            HIP_TRY(ctx, hipMemcpyAsync(hmu.data(), w.mu, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        }
    }
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    if (mean) joint_mean(ctx, w, hmu.data(), mean);
    if (jitter_used) *jitter_used = eps;
    return 0;
}

}  // extern "C"
