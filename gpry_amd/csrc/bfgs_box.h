// The box-constrained BFGS ascent the maximisation kernels share: maxmean_kernel (maximize.hip, the posterior mean) and
// maxacq_kernel (maximize_acq.hip, the LogExp acquisition).  One 256-thread workgroup per start; coordinates are the unit
// cube's, u = (x - lo) / (hi - lo).  The algorithm is a projected BFGS ascent with an Armijo backtracking search, stated
// step by step in include/gpry_hip.h (gpry_maximize_mean) and restated in numpy by tests/tools/maximize_numpy.py: every
// sum runs in the order of the coordinates and every product that feeds a sum goes through ns_rn, so that no FMA fuses
// them.  H (d x d) lives in LDS; H0 is read from global memory at a reset (rare: a change of the free set or a failed
// search).
//
// The objective is a class with
//   double value(const double* x)   the objective at the raw point x (LDS), the same value in every thread; every thread
//                                   calls it (it has barriers)
//   bool ok(double v)               v is a value a state may have (a start that fails it is a BAD_START, a trial that
//                                   fails it is never accepted)
//   void grad(const double* x, double* g)   the unit-cube gradient at the raw point x (LDS) into g (LDS), valid in every
//                                   thread after it; called at a start and at an accepted trial only, which is then the
//                                   last point value() saw
//   void keep()                     the last point value() saw has become the state
//
// Uniformity.  Every barrier is reached by the whole workgroup: every branch around one depends on values that thread 0
// computed and all threads read back from LDS (s_flag, s_free, s_val), or on the objective's value, which is broadcast
// the same way.  Every stop decision is thread 0's.
#pragma once
#include "ns_common.h"

#define BFGS_CONVERGED_G 0
#define BFGS_CONVERGED_F 1
#define BFGS_STALLED 2
#define BFGS_MAXITER 3
#define BFGS_BAD_START 4
#define BFGS_BAD_GRADIENT 5
#define BFGS_C1 1e-4
#define BFGS_CURV 1e-10

// the test hooks: all NULL, or all given (HK = false compiles none of it)
struct BfgsHooks { double* U_tr; double* v_tr; double* G_tr; int* nhalv_tr; int* reset_tr; };
struct BfgsCtl { int max_iter, max_halvings; double gtol, ftol; };
struct BfgsOut {
    double* X_out; double* v_out; double* G_out;
    int* iters; int64_t* ncalls; int64_t* ngrad; int* status;
};

// The ascent of start c = blockIdx.x from the row x0 (d doubles, global); v0: its value, NaN = evaluated here first.
// lo / hi: the box (NsArgs).  Writes row c of every array of `out`.
template <bool HK, class Obj>
__device__ __forceinline__ void bfgs_box_run(Obj& obj, const NsArgs& a, int d, const double* __restrict__ x0, double v0,
                                             const unsigned char* __restrict__ fixed, const double* __restrict__ H0,
                                             const BfgsCtl ctl, const BfgsOut out, const BfgsHooks hk) {
    __shared__ double s_H[GPRY_MAX_DIM * GPRY_MAX_DIM];
    __shared__ double s_x[GPRY_MAX_DIM], s_u[GPRY_MAX_DIM], s_g[GPRY_MAX_DIM];
    __shared__ double s_xt[GPRY_MAX_DIM], s_ut[GPRY_MAX_DIM], s_gt[GPRY_MAX_DIM];
    __shared__ double s_p[GPRY_MAX_DIM];
    __shared__ double s_s[GPRY_MAX_DIM], s_q[GPRY_MAX_DIM], s_hq[GPRY_MAX_DIM];
    __shared__ double s_val[2];
    __shared__ unsigned s_free;
    __shared__ int s_flag;
    const int t = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int max_iter = ctl.max_iter, max_halvings = ctl.max_halvings;
    const double gtol = ctl.gtol, ftol = ctl.ftol;
    unsigned fixm = 0;
    for (int k = 0; k < d; k++) fixm |= fixed[k] ? 1u << k : 0u;
    for (int e = t; e < d * d; e += 256) s_H[e] = H0[e];
    if (t < d) {
        s_x[t] = x0[t];
        s_u[t] = (s_x[t] - a.lo[t]) / (a.hi[t] - a.lo[t]);
        s_g[t] = NAN;
    }
    __syncthreads();
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
            if (t == 0) hk.v_tr[r] = y;
        }
    };
    int64_t n_eval = 0, n_grad = 0;
    int iters = 0, status = BFGS_MAXITER;
    double y_cur = v0;
    if (y_cur != y_cur) {                       // NaN: the start's value is evaluated here
        y_cur = obj.value(s_x);
        n_eval++;
    }
    obj.keep();
    if (t == 0) {
        bool ok = obj.ok(y_cur);
        for (int k = 0; k < d; k++) ok = ok && s_u[k] >= 0.0 && s_u[k] <= 1.0;
        s_flag = ok ? 0 : 1;
    }
    __syncthreads();
    bool run = s_flag == 0;
    __syncthreads();
    if (!run) status = BFGS_BAD_START;
    if (run) {
        obj.grad(s_x, s_g);
        n_grad++;
        if (t == 0) {
            bool fin = true;
            for (int k = 0; k < d; k++) fin = fin && isfinite(s_g[k]);
            s_flag = fin ? 0 : 1;
        }
        __syncthreads();
        if (s_flag) { run = false; status = BFGS_BAD_GRADIENT; }
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
        if (stop) { status = stop == 1 ? BFGS_CONVERGED_G : BFGS_MAXITER; break; }
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
                    s_val[0] = y_cur + ns_rn(BFGS_C1 * ds);
                    s_flag = same ? 1 : 0;
                }
                __syncthreads();
                const bool same = s_flag != 0;
                const double thr = s_val[0];
                __syncthreads();
                if (same) { stalled = true; break; }
                yp = obj.value(s_xt);
                n_eval++;
                if (obj.ok(yp) && yp >= thr) {                  // (yp and thr came through LDS)
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
        if (stalled) { status = BFGS_STALLED; break; }
        // ---- 4. the gradient at the accepted point
        obj.keep();
        obj.grad(s_xt, s_gt);
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
            const bool upd = fin && sq > ns_rn(BFGS_CURV * sqrt(ns_rn(ss * qq)));
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
        if (code & 4) { status = BFGS_BAD_GRADIENT; break; }
        if (code & 2) { status = BFGS_CONVERGED_F; break; }
    }
    if (t < d) {
        out.X_out[c * d + t] = s_x[t];
        out.G_out[c * d + t] = s_g[t];
    }
    if (t == 0) {
        out.v_out[c] = y_cur;
        out.iters[c] = iters;
        out.ncalls[c] = n_eval;
        out.ngrad[c] = n_grad;
        out.status[c] = status;
    }
}

// ---- host side -----------------------------------------------------------------------------------
// What gpry_maximize_mean and gpry_maximize_acq check alike; `hk`: the caller's trace arrays (host pointers).
static int bfgs_check(gpry_ctx* ctx, const char* who, int64_t nstart, const BfgsCtl& ctl, const double* H0, const BfgsHooks& hk) {
    const bool hooks = hk.U_tr != nullptr;
    if ((hk.v_tr != nullptr) != hooks || (hk.G_tr != nullptr) != hooks || (hk.nhalv_tr != nullptr) != hooks ||
        (hk.reset_tr != nullptr) != hooks)
        return gpry_fail(ctx, -1, "%s: the trace hooks are all NULL or all given", who);
    if (nstart < 1 || nstart > 0x7fffffffll || ctl.max_iter < 0 || ctl.max_iter > 100000 || ctl.max_halvings < 0 ||
        ctl.max_halvings > 1000)
        return gpry_fail(ctx, -1, "%s: nstart = %lld, max_iter = %d, max_halvings = %d", who, (long long)nstart, ctl.max_iter,
                         ctl.max_halvings);
    if (!(ctl.gtol >= 0.0) || !isfinite(ctl.gtol)) return gpry_fail(ctx, -1, "%s: gtol = %g", who, ctl.gtol);
    if (!(ctl.ftol >= 0.0) || !isfinite(ctl.ftol)) return gpry_fail(ctx, -1, "%s: ftol = %g", who, ctl.ftol);
    for (int e = 0; e < ctx->d * ctx->d; e++)
        if (!isfinite(H0[e])) return gpry_fail(ctx, -1, "%s: H0 has an entry that is not finite", who);
    return 0;
}

// Declares bfgs_box_run's outputs (`out`: the caller's arrays) and, where given, its traces (`hk`, likewise) on `st`
// behind what the caller has declared, begins the stage and hands back the same two structs with the device's pointers.
// Unused trace slots start as 0xff bytes: NaN and -1.
static int bfgs_begin(NsStage& st, int64_t n, int d, int max_iter, BfgsOut* out, BfgsHooks* hk) {
    const int64_t m1 = max_iter + 1, m0 = max_iter;
    const auto rX = st.out(out->X_out, n * d), rv = st.out(out->v_out, n), rG = st.out(out->G_out, n * d);
    const auto rit = st.out(out->iters, n);
    const auto rnc = st.out(out->ncalls, n), rgr = st.out(out->ngrad, n);
    const auto rst = st.out(out->status, n);
    const auto rU = st.out(hk->U_tr, n * m1 * d, 0xff), rvt = st.out(hk->v_tr, n * m1, 0xff);
    const auto rGt = st.out(hk->G_tr, n * m1 * d, 0xff);
    const auto rnh = st.out(hk->nhalv_tr, n * m0, 0xff), rrs = st.out(hk->reset_tr, n * m0, 0xff);
    GPRY_TRY(st.begin());
    *out = {st.dev(rX), st.dev(rv), st.dev(rG), st.dev(rit), st.dev(rnc), st.dev(rgr), st.dev(rst)};
    *hk = {st.dev(rU), st.dev(rvt), st.dev(rGt), st.dev(rnh), st.dev(rrs)};
    return 0;
}
