// Maximisation of the surrogate's posterior mean on the device: the kernel behind gpry_maximize_mean.  The choice of
// the starts, of H0, the profiles over a grid and their continuation passes are host-side, in gpry_amd/maximize.py.
//
// Objective.  ns_eval of ns_common.h: gpr.predict(x[None]) bit for bit, clip and gates included (a gated point is -inf).
// Gradient.  mean_grad of mean_grad.h, taken to unit-cube coordinates as hmc.hip does (s_gs, grad_at): of the unclipped,
// ungated mean.  No randomness.
//
// One 256-thread workgroup per start; coordinates are the unit cube's, u = (x - lo) / (hi - lo).  The algorithm is a
// projected BFGS ascent with an Armijo backtracking search, stated step by step in include/gpry_hip.h
// (gpry_maximize_mean) and restated in numpy by tests/tools/maximize_numpy.py: every sum runs in the order of the
// coordinates and every product that feeds a sum goes through ns_rn, so that no FMA fuses them.  H (d x d) lives in LDS;
// H0 is read from global memory at a reset (rare: a change of the free set or a failed search).
//
// Uniformity.  Every barrier is reached by the whole workgroup: every branch around one depends on values that thread 0
// computed and all threads read back from LDS (s_flag, s_free, s_val), or on ns_eval's y, which is broadcast the same
// way.  Every stop decision is thread 0's.
#include "ns_common.h"
#include "mean_grad.h"

#define MAXM_CONVERGED_G 0
#define MAXM_CONVERGED_F 1
#define MAXM_STALLED 2
#define MAXM_MAXITER 3
#define MAXM_BAD_START 4
#define MAXM_BAD_GRADIENT 5
#define MAXM_C1 1e-4
#define MAXM_CURV 1e-10

// the test hooks: all NULL, or all given (HK = false compiles none of it)
struct MaxmHooks { double* U_tr; double* y_tr; double* G_tr; int* nhalv_tr; int* reset_tr; };

template <int DP, int KID, bool HK>
__global__ __launch_bounds__(256) void maxmean_kernel(NsArgs a, KernParams kp, AffParams ap, const double* __restrict__ X0,
                                                      const double* __restrict__ y0, const unsigned char* __restrict__ fixed,
                                                      const double* __restrict__ H0, int max_iter, int max_halvings,
                                                      double gtol, double ftol, double minus_inf_value,
                                                      double* __restrict__ X_out, double* __restrict__ y_out,
                                                      double* __restrict__ G_out, int* __restrict__ iters_out,
                                                      int64_t* __restrict__ ncalls, int64_t* __restrict__ ngrad,
                                                      int* __restrict__ status_out, MaxmHooks hk) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_H[GPRY_MAX_DIM * GPRY_MAX_DIM];
    __shared__ double s_gl[MEAN_GRAD_LDS];
    __shared__ double s_x[GPRY_MAX_DIM], s_u[GPRY_MAX_DIM], s_g[GPRY_MAX_DIM];
    __shared__ double s_xt[GPRY_MAX_DIM], s_ut[GPRY_MAX_DIM], s_gt[GPRY_MAX_DIM];
    __shared__ double s_p[GPRY_MAX_DIM], s_xs[GPRY_MAX_DIM], s_gs[GPRY_MAX_DIM];
    __shared__ double s_s[GPRY_MAX_DIM], s_q[GPRY_MAX_DIM], s_hq[GPRY_MAX_DIM];
    __shared__ double s_y, s_val[2];
    __shared__ unsigned s_free;
    __shared__ int s_flag;
    const int t = threadIdx.x, d = kp.d;
    const int64_t c = blockIdx.x;
    unsigned fixm = 0;
    for (int k = 0; k < d; k++) fixm |= fixed[k] ? 1u << k : 0u;
    for (int e = t; e < d * d; e += 256) s_H[e] = H0[e];
    if (t < GPRY_MAX_DIM) {
        s_xs[t] = 0.0;
        s_gs[t] = 0.0;
    }
    if (t < d) {
        s_x[t] = X0[c * d + t];
        s_u[t] = (s_x[t] - a.lo[t]) / (a.hi[t] - a.lo[t]);
        // d y / d u_k over the gradient of the transformed mean in the kernel's coordinates (hmc.hip)
        s_gs[t] = a.y_std * ((a.hi[t] - a.lo[t]) / (kp.has_aff ? ap.span[t] : 1.0));
        s_g[t] = NAN;
    }
    __syncthreads();
    // g (LDS, valid in every thread after it) at the raw point x (LDS)
    auto grad_at = [&](const double* x, double* g) {
        if (t < d) {
            double v = x[t];
            if (kp.has_aff) v = (v - ap.lo[t]) / ap.span[t];
            s_xs[t] = v / ap.ls[t];
        }
        __syncthreads();
        mean_grad<DP, KID>(s_xs, a.Xs, a.alpha_, a.nsplit, a.rows_per_split, kp, ap, s_gl, g);
        if (t < d) g[t] = g[t] * s_gs[t];
        __syncthreads();
    };
    // H = H0 (every thread; a barrier follows)
    auto reset_H = [&]() {
        for (int e = t; e < d * d; e += 256) s_H[e] = H0[e];
        __syncthreads();
    };
    // the state (s_u, y_cur, s_g) into slot i of the traces
    auto trace = [&](int i, double y) {
        if constexpr (HK) {
            const int64_t r = c * (max_iter + 1) + i;
            if (t < d) { hk.U_tr[r * d + t] = s_u[t]; hk.G_tr[r * d + t] = s_g[t]; }
            if (t == 0) hk.y_tr[r] = y;
        }
    };
    int64_t n_eval = 0, n_grad = 0;
    int iters = 0, status = MAXM_MAXITER;
    double y_cur = y0[c];
    if (y_cur != y_cur) {                       // NaN: the start's y is evaluated here
        y_cur = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);
        n_eval++;
    }
    if (t == 0) {
        bool ok = isfinite(y_cur) && y_cur > minus_inf_value;
        for (int k = 0; k < d; k++) ok = ok && s_u[k] >= 0.0 && s_u[k] <= 1.0;
        s_flag = ok ? 0 : 1;
    }
    __syncthreads();
    bool run = s_flag == 0;
    __syncthreads();
    if (!run) status = MAXM_BAD_START;
    if (run) {
        grad_at(s_x, s_g);
        n_grad++;
        if (t == 0) {
            bool fin = true;
            for (int k = 0; k < d; k++) fin = fin && isfinite(s_g[k]);
            s_flag = fin ? 0 : 1;
        }
        __syncthreads();
        if (s_flag) { run = false; status = MAXM_BAD_GRADIENT; }
        __syncthreads();
    }
    trace(0, y_cur);
    bool h0 = true;                             // H is H0
    unsigned prev_free = 0;
    bool first = true;                          // (no iteration yet: the first free set is no change)
    while (run) {
        // ---- 1. the free set and the gradient test
        if (t == 0) {
            unsigned fm = 0;
            double gmax = 0.0;
            for (int k = 0; k < d; k++) {
                const bool fr = !(fixm >> k & 1u) && !(s_u[k] == 0.0 && s_g[k] <= 0.0) && !(s_u[k] == 1.0 && s_g[k] >= 0.0);
                if (fr) { fm |= 1u << k; gmax = fmax(gmax, fabs(s_g[k])); }
            }
            s_free = fm;
            s_flag = (fm == 0u || gmax <= gtol) ? 1 : (iters >= max_iter ? 2 : 0);
        }
        __syncthreads();
        const unsigned fm = s_free;
        const int stop = s_flag;
        __syncthreads();
        if (stop) { status = stop == 1 ? MAXM_CONVERGED_G : MAXM_MAXITER; break; }
        int nreset = 0, nhalv = -1;
        // ---- 2. a changed free set forgets the curvature
        if (!first && fm != prev_free && !h0) {
            reset_H();
            h0 = true;
            nreset++;
        }
        prev_free = fm;
        first = false;
        const bool fr_t = t < d && (fm >> t & 1u);
        double yp = NAN;
        bool accepted = false, stalled = false;
        for (;;) {                              // direction and search; once more after a reset of H
            if (t < d) {
                double v = 0.0;
                if (fr_t)
                    for (int j = 0; j < d; j++)
                        if (fm >> j & 1u) v = v + ns_rn(s_H[t * d + j] * s_g[j]);
                s_p[t] = v;
            }
            __syncthreads();
            if (t == 0) {
                double pg = 0.0;
                for (int k = 0; k < d; k++)
                    if (fm >> k & 1u) pg = pg + ns_rn(s_p[k] * s_g[k]);
                s_flag = pg > 0.0 ? 1 : 0;
            }
            __syncthreads();
            const bool ascent = s_flag != 0;
            __syncthreads();
            if (!ascent) {
                if (h0) { stalled = true; break; }
                reset_H();
                h0 = true;
                nreset++;
                continue;
            }
            // ---- 3. Armijo backtracking
            double ts = 1.0;
            for (int h = 0; h <= max_halvings; h++) {
                if (t < d) {
                    double un = s_u[t], xn = s_x[t];
                    if (fr_t) {
                        un = s_u[t] + ns_rn(ts * s_p[t]);
                        un = un < 0.0 ? 0.0 : (un > 1.0 ? 1.0 : un);
                        if (un != s_u[t]) {
                            xn = a.lo[t] + ns_rn(un * (a.hi[t] - a.lo[t]));
                            xn = xn < a.lo[t] ? a.lo[t] : (xn > a.hi[t] ? a.hi[t] : xn);
                            if (un == 1.0) xn = a.hi[t];        // (lo + (hi - lo) may miss hi by an ulp)
                        }
                    }
                    s_ut[t] = un;
                    s_xt[t] = xn;
                }
                __syncthreads();
                if (t == 0) {
                    bool same = true;
                    double ds = 0.0;
                    for (int k = 0; k < d; k++) {
                        same = same && s_ut[k] == s_u[k];
                        if (fm >> k & 1u) ds = ds + ns_rn(s_g[k] * (s_ut[k] - s_u[k]));
                    }
                    s_val[0] = y_cur + ns_rn(MAXM_C1 * ds);
                    s_flag = same ? 1 : 0;
                }
                __syncthreads();
                const bool same = s_flag != 0;
                const double thr = s_val[0];
                __syncthreads();
                if (same) { stalled = true; break; }
                yp = ns_eval<DP, KID>(s_xt, a, kp, ap, r2s, red, &s_y);
                n_eval++;
                if (isfinite(yp) && yp > minus_inf_value && yp >= thr) {        // (yp and thr came through LDS)
                    accepted = true;
                    nhalv = h;
                    break;
                }
                ts = ts * 0.5;
            }
            if (accepted || stalled) break;
            if (h0) { stalled = true; break; }
            reset_H();
            h0 = true;
            nreset++;
        }
        if constexpr (HK) {
            if (t == 0) {
                hk.nhalv_tr[c * max_iter + iters] = nhalv;
                hk.reset_tr[c * max_iter + iters] = nreset;
            }
        }
        if (stalled) { status = MAXM_STALLED; break; }
        // ---- 4. the gradient at the accepted point
        grad_at(s_xt, s_gt);
        n_grad++;
        if (t < d) {
            s_s[t] = fr_t ? s_ut[t] - s_u[t] : 0.0;
            s_q[t] = fr_t ? s_g[t] - s_gt[t] : 0.0;
        }
        __syncthreads();
        // ---- 5. the BFGS update of the free block
        if (t < d) {
            double v = 0.0;
            if (fr_t)
                for (int j = 0; j < d; j++)
                    if (fm >> j & 1u) v = v + ns_rn(s_H[t * d + j] * s_q[j]);
            s_hq[t] = v;
        }
        __syncthreads();
        if (t == 0) {
            bool fin = true;
            double sq = 0.0, ss = 0.0, qq = 0.0, qhq = 0.0;
            for (int k = 0; k < d; k++) {
                fin = fin && isfinite(s_gt[k]);
                sq = sq + ns_rn(s_s[k] * s_q[k]);
                ss = ss + ns_rn(s_s[k] * s_s[k]);
                qq = qq + ns_rn(s_q[k] * s_q[k]);
                qhq = qhq + ns_rn(s_q[k] * s_hq[k]);
            }
            const bool upd = fin && sq > ns_rn(MAXM_CURV * sqrt(ns_rn(ss * qq)));
            const double rho = 1.0 / sq;
            s_val[0] = rho;
            s_val[1] = ns_rn(ns_rn(rho * rho) * qhq) + rho;
            // 6. the stops after an accepted step
            s_flag = !fin ? 4 : ((yp - y_cur <= ns_rn(ftol * fmax(1.0, fabs(yp))) ? 2 : 0) | (upd ? 1 : 0));
        }
        __syncthreads();
        const int code = s_flag;
        const double rho = s_val[0], c2 = s_val[1];
        if (code & 1) {
            for (int e = t; e < d * d; e += 256) {
                const int k = e / d, j = e % d;
                if ((fm >> k & 1u) && (fm >> j & 1u))
                    s_H[e] = (s_H[e] - ns_rn(rho * (ns_rn(s_s[k] * s_hq[j]) + ns_rn(s_hq[k] * s_s[j]))))
                             + ns_rn(c2 * ns_rn(s_s[k] * s_s[j]));
            }
            h0 = false;
        }
        __syncthreads();
        // the accepted point becomes the state
        if (t < d) { s_u[t] = s_ut[t]; s_x[t] = s_xt[t]; s_g[t] = s_gt[t]; }
        y_cur = yp;
        iters++;
        __syncthreads();
        trace(iters, y_cur);
        if (code & 4) { status = MAXM_BAD_GRADIENT; break; }
        if (code & 2) { status = MAXM_CONVERGED_F; break; }
    }
    if (t < d) {
        X_out[c * d + t] = s_x[t];
        G_out[c * d + t] = s_g[t];
    }
    if (t == 0) {
        y_out[c] = y_cur;
        iters_out[c] = iters;
        ncalls[c] = n_eval;
        ngrad[c] = n_grad;
        status_out[c] = status;
    }
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
    const bool hooks = U_tr != nullptr;
    if ((y_tr != nullptr) != hooks || (G_tr != nullptr) != hooks || (nhalv_tr != nullptr) != hooks ||
        (reset_tr != nullptr) != hooks)
        return gpry_fail(ctx, -1, "gpry_maximize_mean: the trace hooks are all NULL or all given");
    if (nstart < 1 || nstart > 0x7fffffffll || max_iter < 0 || max_iter > 100000 || max_halvings < 0 || max_halvings > 1000)
        return gpry_fail(ctx, -1, "gpry_maximize_mean: nstart = %lld, max_iter = %d, max_halvings = %d",
                         (long long)nstart, max_iter, max_halvings);
    if (!(gtol >= 0.0) || !isfinite(gtol)) return gpry_fail(ctx, -1, "gpry_maximize_mean: gtol = %g", gtol);
    if (!(ftol >= 0.0) || !isfinite(ftol)) return gpry_fail(ctx, -1, "gpry_maximize_mean: ftol = %g", ftol);
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_maximize_mean", lo, hi, 0, &a, &kp, &ap));
    const int d = ctx->d;
    for (int e = 0; e < d * d; e++)
        if (!isfinite(H0[e])) return gpry_fail(ctx, -1, "gpry_maximize_mean: H0 has an entry that is not finite");
    const int64_t n = nstart, m1 = max_iter + 1, m0 = max_iter;
    // one buffer: [X0 | y0 | H0 | fixed | X_out | y_out | G_out | iters | ncalls | ngrad | status | U_tr | y_tr | G_tr |
    //              nhalv_tr | reset_tr], a hook's region empty unless asked for
    const int64_t sz[16] = {8 * n * d, 8 * n, 8 * (int64_t)d * d, d, 8 * n * d, 8 * n, 8 * n * d, 4 * n, 8 * n, 8 * n, 4 * n,
                            hooks ? 8 * n * m1 * d : 0, hooks ? 8 * n * m1 : 0, hooks ? 8 * n * m1 * d : 0,
                            hooks ? 4 * n * m0 : 0, hooks ? 4 * n * m0 : 0};
    int64_t off[17];
    ns_layout(sz, off);
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    GPRY_TRY(dev_grow(ctx, &ctx->dmc, &ctx->mc_cap, off[16]));
    char* b = (char*)ctx->dmc;
    const void* src[4] = {X0, y0, H0, fixed};
    for (int i = 0; i < 4; i++) HIP_TRY(ctx, hipMemcpyAsync(b + off[i], src[i], sz[i], hipMemcpyHostToDevice, ctx->stream));
    // unused trace slots: NaN (all bits set) and -1
    if (hooks) HIP_TRY(ctx, hipMemsetAsync(b + off[11], 0xff, off[16] - off[11], ctx->stream));
    const double* dX0 = (const double*)(b + off[0]);
    const double* dy0 = (const double*)(b + off[1]);
    const double* dH0 = (const double*)(b + off[2]);
    const unsigned char* dfx = (const unsigned char*)(b + off[3]);
    double* dXo = (double*)(b + off[4]);
    double* dyo = (double*)(b + off[5]);
    double* dGo = (double*)(b + off[6]);
    int* dit = (int*)(b + off[7]);
    int64_t* dnc = (int64_t*)(b + off[8]);
    int64_t* dng = (int64_t*)(b + off[9]);
    int* dst_ = (int*)(b + off[10]);
    MaxmHooks hk = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (hooks) hk = {(double*)(b + off[11]), (double*)(b + off[12]), (double*)(b + off[13]), (int*)(b + off[14]), (int*)(b + off[15])};
#define MX(DP, KID, HK)                                                                                                   \
    hipLaunchKernelGGL((maxmean_kernel<DP, KID, HK>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap, dX0, dy0, dfx, \
                       dH0, max_iter, max_halvings, gtol, ftol, minus_inf_value, dXo, dyo, dGo, dit, dnc, dng, dst_, hk)
#define MX_PLAIN(DP, KID) MX(DP, KID, false)
#define MX_HOOKS(DP, KID) MX(DP, KID, true)
    if (hooks) { DISPATCH_DP_KID(d, ctx->kernel_id, MX_HOOKS) }
    else { DISPATCH_DP_KID(d, ctx->kernel_id, MX_PLAIN) }
#undef MX_HOOKS
#undef MX_PLAIN
#undef MX
    HIP_TRY(ctx, hipGetLastError());
    void* dst[12] = {X_out, y_out, G_out, iters, ncalls, ngrad, status, U_tr, y_tr, G_tr, nhalv_tr, reset_tr};
    for (int i = 4; i < 16; i++)
        if (sz[i] > 0) HIP_TRY(ctx, hipMemcpyAsync(dst[i - 4], b + off[i], sz[i], hipMemcpyDeviceToHost, ctx->stream));
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    return 0;
}

}  // extern "C"
