// Maximisation of the surrogate's posterior mean on the device: the kernel behind gpry_maximize_mean.  The choice of
// the starts, of H0, the profiles over a grid and their continuation passes are host-side, in gpry_amd/maximize.py.
//
// Objective.  ns_eval of ns_common.h: gpr.predict(x[None]) bit for bit, clip and gates included (a gated point is -inf).
// Gradient.  mean_grad of mean_grad.h, taken to unit-cube coordinates as hmc.hip does (s_gs, grad): of the unclipped,
// ungated mean.  No randomness.
//
// The ascent itself -- one 256-thread workgroup per start, a projected BFGS ascent with an Armijo backtracking search in
// the unit cube, stated step by step in include/gpry_hip.h (gpry_maximize_mean) -- is bfgs_box_run of bfgs_box.h, shared
// with maximize_acq.hip; this file gives it the mean as objective.
#include "bfgs_box.h"
#include "mean_grad.h"

// the mean as bfgs_box_run's objective
template <int DP, int KID>
struct MeanObjective {
    const NsArgs& a; const KernParams& kp; const AffParams& ap;
    double minus_inf_value;
    double *r2s, *red, *s_gl, *s_xs, *s_gs, *s_y;
    __device__ __forceinline__ double value(const double* x) { return ns_eval<DP, KID>(x, a, kp, ap, r2s, red, s_y); }
    __device__ __forceinline__ bool ok(double v) const { return isfinite(v) && v > minus_inf_value; }
    // g (LDS, valid in every thread after it) at the raw point x (LDS)
    __device__ __forceinline__ void grad(const double* x, double* g) {
        const int t = threadIdx.x, d = kp.d;
        if (t < d) {
            double v = x[t];
            if (kp.has_aff) v = (v - ap.lo[t]) / ap.span[t];
            s_xs[t] = v / ap.ls[t];
        }
        __syncthreads();
        mean_grad<DP, KID>(s_xs, a.Xs, a.alpha_, a.nsplit, a.rows_per_split, kp, ap, s_gl, g);
        if (t < d) g[t] = g[t] * s_gs[t];
        __syncthreads();
    }
    __device__ __forceinline__ void keep() {}
};

template <int DP, int KID, bool HK>
__global__ __launch_bounds__(256) void maxmean_kernel(NsArgs a, KernParams kp, AffParams ap, const double* __restrict__ X0,
                                                      const double* __restrict__ y0, const unsigned char* __restrict__ fixed,
                                                      const double* __restrict__ H0, BfgsCtl ctl, double minus_inf_value,
                                                      BfgsOut out, BfgsHooks hk) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_gl[MEAN_GRAD_LDS];
    __shared__ double s_xs[GPRY_MAX_DIM], s_gs[GPRY_MAX_DIM];
    __shared__ double s_y;
    const int t = threadIdx.x, d = kp.d;
    const int64_t c = blockIdx.x;
    if (t < GPRY_MAX_DIM) {
        s_xs[t] = 0.0;
        // d y / d u_k over the gradient of the transformed mean in the kernel's coordinates (hmc.hip)
        s_gs[t] = t < d ? a.y_std * ((a.hi[t] - a.lo[t]) / (kp.has_aff ? ap.span[t] : 1.0)) : 0.0;
    }
    MeanObjective<DP, KID> obj{a, kp, ap, minus_inf_value, r2s, red, s_gl, s_xs, s_gs, &s_y};
    bfgs_box_run<HK>(obj, a, d, X0 + c * d, y0[c], fixed, H0, ctl, out, hk);      // (its first barrier covers s_xs, s_gs)
}

extern "C" {

int gpry_maximize_mean(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                       int64_t nstart, const unsigned char* fixed, const double* H0, int max_iter, int max_halvings,
                       double gtol, double ftol, double minus_inf_value, double* X_out, double* y_out, double* G_out,
                       int* iters, int64_t* ncalls, int64_t* ngrad, int* status, double* U_tr, double* y_tr, double* G_tr,
                       int* nhalv_tr, int* reset_tr, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_maximize_mean: ctx is NULL");
    if (!lo || !hi || !X0 || !y0 || !fixed || !H0 || !X_out || !y_out || !G_out || !iters || !ncalls || !ngrad || !status)
        return gpry_fail(ctx, -1, "gpry_maximize_mean: NULL argument");
    const BfgsCtl ctl = {max_iter, max_halvings, gtol, ftol};
    BfgsOut out = {X_out, y_out, G_out, iters, ncalls, ngrad, status};
    BfgsHooks hk = {U_tr, y_tr, G_tr, nhalv_tr, reset_tr};
    const bool hooks = U_tr != nullptr;
    GPRY_TRY(bfgs_check(ctx, "gpry_maximize_mean", nstart, ctl, H0, hk));
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_maximize_mean", lo, hi, 0, &a, &kp, &ap));
    const int d = ctx->d;
    const int64_t n = nstart;
    NsStage st(ctx);
    const auto rX0 = st.in(X0, n * d), ry0 = st.in(y0, n), rH0 = st.in(H0, (int64_t)d * d);
    const auto rfx = st.in(fixed, d);
    GPRY_TRY(bfgs_begin(st, n, d, max_iter, &out, &hk));
#define MX(DP, KID, HK)                                                                                                   \
    hipLaunchKernelGGL((maxmean_kernel<DP, KID, HK>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap, st.dev(rX0), \
                       st.dev(ry0), st.dev(rfx), st.dev(rH0), ctl, minus_inf_value, out, hk)
#define MX_PLAIN(DP, KID) MX(DP, KID, false)
#define MX_HOOKS(DP, KID) MX(DP, KID, true)
    if (hooks) { DISPATCH_DP_KID(d, ctx->kernel_id, MX_HOOKS) }
    else { DISPATCH_DP_KID(d, ctx->kernel_id, MX_PLAIN) }
#undef MX_HOOKS
#undef MX_PLAIN
#undef MX
    return st.end(device_ms);
}

}  // extern "C"
