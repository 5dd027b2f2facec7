// Maximisation of the LogExp acquisition on the device: the kernel behind gpry_maximize_acq.  The choice of the starts
// and of H0 is host-side, in gpry_amd/maximize.py (maximize_acq) and gpry_amd/gp_acquisition.py (BatchOptimizer with
// acq_optimizer="device").  The ascent is bfgs_box_run of bfgs_box.h, the one maximize.hip runs on the mean; this file
// gives it a(x) = logexp_value(y, sigma) as objective, with its exact gradient.  No randomness, no atomics.
//
// Value of one point x (raw coordinates, LDS), by the whole workgroup:
//   y       ns_eval: gpr.predict(x[None]) bit for bit, clip and gates included
//   k*_j    C kappa(r_j), j < N, difference form on the scaled rows Xs that mean_slice reads; into LDS (r2s, which
//           ns_eval has finished with)
//   pass 1  u = V k*, V = L^-1 row-major with leading dimension Np, lower triangular: row i over the columns 0 .. i only.
//           A wave takes four rows at a time, its lanes stride the columns in pairs (16-byte loads), one partial sum per
//           row and lane (columns 2 lane, 2 lane + 1, 2 lane + 128, ... in ascending order), reduced across the lanes by
//           offsets 32, 16, ..., 1.  u_i into LDS.
//           Rows and columns >= N are never read (the pad rows of V hold what the last factorisation or border update
//           left there).
//   ss      sum u_i^2: thread t over i = t, t + 256, ..., then mean_slice's tree over the 256 partial sums
//   sigma   finish_sd: sqrt(max(C - ss, 0)) y_std, 0 under the classifier bit of the device gates
//   a       logexp_value(y, sigma, zeta, baseline, sigma_n); -inf unless y is finite, y > minus_inf_value and
//           dv = rn(sigma sigma) - rn(sigma_n sigma_n) > 0
// Gradient, at a start and at an accepted trial only (the last point the value saw: its u, scaled coordinates and dv
// are still in LDS, pass 1 is not repeated):
//   pass 2  w = V^T u (= K^-1 k*): a wave owns a block of 128 columns, lane l the columns j = 128 b + 2 l and j + 1, and
//           walks the rows i = 128 b .. N - 1 (i >= column only), reading 1024-byte row segments; u_i is broadcast from
//           LDS; four partial sums per column (rows i = 0, 1, 2, 3 mod 4 from the block's first row) added as
//           (s0 + s1) + (s2 + s3).  w into LDS (over k*, which pass 1 has finished with).
//   m = G^T alpha_, v = G^T w   mean_grad of mean_grad.h, twice (with alpha_, and with w in its place)
//   g_k = s_k (rn(rn((2 zeta) y_std) m_k) + rn(rn(y_std y_std) (-v_k)) / dv),  s_k = (hi_k - lo_k) / x_span_k
// which is the gradient of a with respect to the unit cube: d sigma_^2 / dx = -2 G^T w in the kernel's coordinates.
//
// LDS: the static arrays of the mean kernel and, dynamic, Np doubles for u.
#include "bfgs_box.h"
#include "mean_grad.h"
#include "acq_math.h"

#define MAXACQ_NP_MAX 4096

struct AcqParams {
    const double* V; int64_t ldv;
    double zeta, baseline, sigma_n, minus_inf_value;
};

// the acquisition as bfgs_box_run's objective
template <int DP, int KID>
struct AcqObjective {
    const NsArgs& a; const KernParams& kp; const AffParams& ap; const AcqParams& q;
    double *r2s, *red, *s_gl, *s_xs, *s_sc, *s_gm, *s_gv, *s_y, *s_av, *uvec;
    double y_last = NAN, sd_last = NAN, dv_last = NAN, y_cur = NAN, sd_cur = NAN;

    __device__ __forceinline__ bool ok(double v) const { return isfinite(v); }
    __device__ __forceinline__ void keep() { y_cur = y_last; sd_cur = sd_last; }

    __device__ __forceinline__ double value(const double* x) {
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6, d = kp.d;
        const int N = (int)kp.N;
        const double y = ns_eval<DP, KID>(x, a, kp, ap, r2s, red, s_y);
        // which gate it was decides sigma (the classifier's verdict zeroes it): asked again for the few points that are gated
        unsigned bits = 0;
        if (a.gates && y == -INFINITY) bits = point_gate_bits(x, a.gate, kp, ap, red);
        if (t < d) {
            double v = x[t];
            if (kp.has_aff) v = (v - ap.lo[t]) / ap.span[t];
            s_xs[t] = v / ap.ls[t];
        }
        __syncthreads();
        // ---- k* (difference form), one row per thread
        double* kst = r2s;
        {
            constexpr int P = DP / 2;
            double xr[DP];
#pragma unroll
            for (int k = 0; k < DP; k++) xr[k] = s_xs[k];
            for (int j = t; j < N; j += 256) {
                double r2 = 0.0;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    double2 v = make_double2(0.0, 0.0);
                    if (2 * p < kp.dpad) v = *reinterpret_cast<const double2*>(a.Xs + (int64_t)j * kp.dpad + 2 * p);
                    const double d0 = 2 * p < d ? xr[2 * p] - v.x : 0.0;
                    const double d1 = 2 * p + 1 < d ? xr[2 * p + 1] - v.y : 0.0;
                    r2 = fma(d0, d0, r2);
                    r2 = fma(d1, d1, r2);
                }
                kst[j] = kp.C * corr_r2_fast<KID>(r2);
            }
        }
        __syncthreads();
        // ---- pass 1: u = V k* (16-byte loads: a lane takes the columns 2 lane, 2 lane + 1 of every 128)
        for (int i0 = 4 * wave; i0 < N; i0 += 16) {
            const int imax = i0 + 3 < N ? i0 + 3 : N - 1;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c0 = 2 * lane; c0 <= imax; c0 += 512) {
                double2 v[4][4], kk[4];
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const int c = c0 + 128 * s;         // (even, so c + 1 < Np whenever c < Np: the pair is inside its row)
                    kk[s] = make_double2(0.0, 0.0);
                    if (c <= imax) kk[s] = *reinterpret_cast<const double2*>(kst + c);
                    if (c + 1 > imax) kk[s].y = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        v[r][s] = make_double2(0.0, 0.0);
                        if (c <= i0 + r && i0 + r < N) v[r][s] = *reinterpret_cast<const double2*>(q.V + (int64_t)(i0 + r) * q.ldv + c);
                        if (c + 1 > i0 + r) v[r][s].y = 0.0;        // (above the diagonal: not part of the row's sum)
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; s++)
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[r] = fma(v[r][s].y, kk[s].y, fma(v[r][s].x, kk[s].x, acc[r]));
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double s = acc[r];
                s += __shfl_down(s, 32);
                s += __shfl_down(s, 16);
                s += __shfl_down(s, 8);
                s += __shfl_down(s, 4);
                s += __shfl_down(s, 2);
                s += __shfl_down(s, 1);
                if (lane == 0 && i0 + r < N) uvec[i0 + r] = s;
            }
        }
        __syncthreads();
        // ---- ss = |u|^2 and the finish
        double part = 0.0;
        for (int i = t; i < N; i += 256) part = fma(uvec[i], uvec[i], part);
        red[t] = part;
        __syncthreads();
        if (t < 64) {
            double ss = (red[t] + red[t + 128]) + (red[t + 64] + red[t + 192]);
            ss += __shfl_down(ss, 32);
            ss += __shfl_down(ss, 16);
            ss += __shfl_down(ss, 8);
            ss += __shfl_down(ss, 4);
            ss += __shfl_down(ss, 2);
            ss += __shfl_down(ss, 1);
            if (t == 0) {
                FinishParams fp = {};
                fp.C = kp.C;
                fp.y_std = a.y_std;
                const double sd = finish_sd(ss, bits, fp);
                double av = logexp_value(y, sd, q.zeta, q.baseline, q.sigma_n);
                const double dv = ns_rn(sd * sd) - ns_rn(q.sigma_n * q.sigma_n);
                if (!(isfinite(y) && y > q.minus_inf_value && dv > 0.0)) av = -INFINITY;
                s_av[0] = av;
                s_av[1] = sd;
                s_av[2] = dv;
            }
        }
        __syncthreads();
        const double av = s_av[0];
        y_last = y;
        sd_last = s_av[1];
        dv_last = s_av[2];
        __syncthreads();
        return av;
    }

    // g (LDS, valid in every thread after it) at the point value() saw last (x is that point)
    __device__ __forceinline__ void grad(const double* x, double* g) {
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6, d = kp.d;
        const int N = (int)kp.N;
        double* wvec = r2s;
        // ---- pass 2: w = V^T u (16-byte loads: a wave owns 128 columns, a lane two of them)
        const int nblk = (N + 127) / 128;
        for (int r = 0; 4 * r < nblk; r++) {
            const int b = 4 * r + ((r & 1) ? 3 - wave : wave);      // (the long and the short blocks alternate over the waves)
            if (b >= nblk) continue;
            const int j = 128 * b + 2 * lane;           // (even: the pair j, j + 1 is inside its row whenever j < N <= Np)
            const bool col = j < N;
            double ax[4] = {0.0, 0.0, 0.0, 0.0}, ay[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i0 = 128 * b; i0 < N; i0 += 16) {
                double2 v[16];
                double uu[16];
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    const int i = i0 + s;
                    uu[s] = i < N ? uvec[i] : 0.0;
                    v[s] = make_double2(0.0, 0.0);
                    if (col && i < N && i >= j) v[s] = *reinterpret_cast<const double2*>(q.V + (int64_t)i * q.ldv + j);
                    if (i < j + 1 || j + 1 >= N) v[s].y = 0.0;      // (above the diagonal, or past the last column)
                }
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    ax[s & 3] = fma(v[s].x, uu[s], ax[s & 3]);
                    ay[s & 3] = fma(v[s].y, uu[s], ay[s & 3]);
                }
            }
            if (col) wvec[j] = (ax[0] + ax[1]) + (ax[2] + ax[3]);
            if (j + 1 < N) wvec[j + 1] = (ay[0] + ay[1]) + (ay[2] + ay[3]);
        }
        __syncthreads();
        mean_grad<DP, KID>(s_xs, a.Xs, wvec, a.nsplit, a.rows_per_split, kp, ap, s_gl, s_gv);
        mean_grad<DP, KID>(s_xs, a.Xs, a.alpha_, a.nsplit, a.rows_per_split, kp, ap, s_gl, s_gm);
        if (t < d) {
            const double t1 = ns_rn(ns_rn((2.0 * q.zeta) * a.y_std) * s_gm[t]);
            const double t2 = ns_rn(ns_rn(a.y_std * a.y_std) * (-s_gv[t])) / dv_last;
            g[t] = s_sc[t] * (t1 + t2);
        }
        __syncthreads();
    }
};

template <int DP, int KID, bool HK>
__global__ __launch_bounds__(256) void maxacq_kernel(NsArgs a, KernParams kp, AffParams ap, AcqParams q,
                                                     const double* __restrict__ X0, const unsigned char* __restrict__ fixed,
                                                     const double* __restrict__ H0, BfgsCtl ctl, BfgsOut out,
                                                     double* __restrict__ y_out, double* __restrict__ sigma_out, BfgsHooks hk) {
    extern __shared__ double s_dyn[];           // u: Np doubles
    __shared__ __attribute__((aligned(16))) double r2s[MEAN_SLICE_CH];   // ns_eval's distances, then k*, then w (read in pairs)
    __shared__ double red[256];
    __shared__ double s_gl[MEAN_GRAD_LDS];
    __shared__ double s_xs[GPRY_MAX_DIM], s_sc[GPRY_MAX_DIM], s_gm[GPRY_MAX_DIM], s_gv[GPRY_MAX_DIM];
    __shared__ double s_y, s_av[3];
    const int t = threadIdx.x, d = kp.d;
    const int64_t c = blockIdx.x;
    if (t < GPRY_MAX_DIM) {
        s_xs[t] = 0.0;
        s_sc[t] = t < d ? (a.hi[t] - a.lo[t]) / (kp.has_aff ? ap.span[t] : 1.0) : 0.0;
    }
    AcqObjective<DP, KID> obj{a, kp, ap, q, r2s, red, s_gl, s_xs, s_sc, s_gm, s_gv, &s_y, s_av, s_dyn};
    bfgs_box_run<HK>(obj, a, d, X0 + c * d, NAN, fixed, H0, ctl, out, hk);        // (its first barrier covers s_xs, s_sc)
    if (t == 0) {
        y_out[c] = obj.y_cur;
        sigma_out[c] = obj.sd_cur;
    }
}

extern "C" {

int gpry_maximize_acq(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, int64_t nstart,
                      const unsigned char* fixed, const double* H0, double zeta, double baseline, double sigma_n,
                      int max_iter, int max_halvings, double gtol, double ftol, double minus_inf_value, double* X_out,
                      double* a_out, double* y_out, double* sigma_out, double* G_out, int* iters, int64_t* ncalls,
                      int64_t* ngrad, int* status, double* U_tr, double* a_tr, double* G_tr, int* nhalv_tr, int* reset_tr,
                      double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_maximize_acq: ctx is NULL");
    if (!lo || !hi || !X0 || !fixed || !H0 || !X_out || !a_out || !y_out || !sigma_out || !G_out || !iters || !ncalls ||
        !ngrad || !status)
        return gpry_fail(ctx, -1, "gpry_maximize_acq: NULL argument");
    const BfgsCtl ctl = {max_iter, max_halvings, gtol, ftol};
    BfgsOut out = {X_out, a_out, G_out, iters, ncalls, ngrad, status};
    BfgsHooks hk = {U_tr, a_tr, G_tr, nhalv_tr, reset_tr};
    const bool hooks = U_tr != nullptr;
    GPRY_TRY(bfgs_check(ctx, "gpry_maximize_acq", nstart, ctl, H0, hk));
    if (!(sigma_n >= 0.0) || !isfinite(sigma_n)) return gpry_fail(ctx, -1, "gpry_maximize_acq: sigma_n = %g", sigma_n);
    if (!isfinite(zeta) || !isfinite(baseline))
        return gpry_fail(ctx, -1, "gpry_maximize_acq: zeta = %g, baseline = %g", zeta, baseline);
    GPRY_TRY(require_model(ctx, true));
    GPRY_TRY(refuse_white(ctx, "gpry_maximize_acq"));
    if (ctx->Np > MAXACQ_NP_MAX)
        return gpry_fail(ctx, -1, "gpry_maximize_acq: the model has %lld padded rows, more than %d", (long long)ctx->Np,
                         MAXACQ_NP_MAX);
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_maximize_acq", lo, hi, 0, &a, &kp, &ap));
    const int d = ctx->d;
    const int64_t n = nstart;
    NsStage st(ctx);
    const auto rX0 = st.in(X0, n * d), rH0 = st.in(H0, (int64_t)d * d);
    const auto rfx = st.in(fixed, d);
    const auto ryo = st.out(y_out, n), rso = st.out(sigma_out, n);
    GPRY_TRY(bfgs_begin(st, n, d, max_iter, &out, &hk));
    const AcqParams q = {ctx->dV, ctx->Np, zeta, baseline, sigma_n, minus_inf_value};
    const int lds = (int)(8 * ctx->Np);         // with the static arrays above 64 KB from Np = 2048 on
#define MA(DP, KID, HK)                                                                                                   \
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)maxacq_kernel<DP, KID, HK>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                     lds));                                                                               \
    hipLaunchKernelGGL((maxacq_kernel<DP, KID, HK>), dim3((unsigned)n), dim3(256), lds, ctx->stream, a, kp, ap, q,           \
                       st.dev(rX0), st.dev(rfx), st.dev(rH0), ctl, out, st.dev(ryo), st.dev(rso), hk)
#define MA_PLAIN(DP, KID) MA(DP, KID, false)
#define MA_HOOKS(DP, KID) MA(DP, KID, true)
    if (hooks) { DISPATCH_DP_KID(d, ctx->kernel_id, MA_HOOKS) }
    else { DISPATCH_DP_KID(d, ctx->kernel_id, MA_PLAIN) }
#undef MA_HOOKS
#undef MA_PLAIN
#undef MA
    return st.end(device_ms);
}

}  // extern "C"
