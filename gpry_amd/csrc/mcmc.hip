// Metropolis MCMC of the surrogate's posterior mean on the device: the kernel behind gpry_mcmc_chains.  The adaptation
// of the proposal, the convergence test (R - 1 over split chains), the burn-in and the temperature weights are host-side,
// in gpry_amd/mcmc.py; together they replace the Cobaya MCMC runs of gpry/mc.py:173-327 (the surrogate's final sample),
// gpry/convergence.py:430-476 (GaussianKL's MC fallback) and gpry/proposal.py:359-443 (SmallChainProposer), which call
// gpr.predict once per point.
//
// Likelihood.  ns_eval of ns_common.h: gpr.predict(x[None]) bit for bit, gates included (-inf where they reject).
//
// Randomness.  ns_philox with phase 3: step s of chain c in call `batch` takes the counters (3, draw j, batch, c, s);
// draws 0..15 give z ~ N(0, I) by Box-Muller (ns_box_muller of ns_common.h, which ns_chain_kernel calls too), draw 16
// gives the acceptance uniform ua.  No value depends on how many chains share a launch or on the workgroup schedule.
//
// Chains.  One 256-thread workgroup per chain, `nsteps` Metropolis steps inside the kernel.  Coordinates are the unit
// cube's, u = (x - lo) / (hi - lo); the proposal is u' = u + Lp z (Lp: lower triangular, scale included).  A proposal
// outside the box (the test of ns_chain_kernel's try_at) is rejected without an evaluation; otherwise y' = ns_eval(x')
// and the step is accepted iff y' is finite, y' > minus_inf_value and log(1 - ua) < (y' - y) / T.  Every product that
// feeds a sum goes through ns_rn, so that no FMA fuses them (-ffp-contract=fast) and the host can restate the step.
#include "ns_common.h"

#define MC_PHASE 3u
#define MC_DRAW_ACCEPT 16u          // draws 0..15 of a step: z; draw 16: the acceptance uniform

// Outputs, per chain c: the state after every thin-th step (X_rec: nrec x d, y_rec: nrec, nrec = nsteps / thin), the
// final state, the accepted steps and the evaluations (the start's included when y0[c] is NaN: it is evaluated first).
// Test hook (X_prop non-NULL): every proposal and its y, NaN where it was not evaluated (outside the box).
template <int DP, int KID>
__global__ __launch_bounds__(256) void mcmc_chain_kernel(NsArgs a, KernParams kp, AffParams ap,
                                                         const double* __restrict__ X0, const double* __restrict__ y0,
                                                         const double* __restrict__ Lp, double T, double minus_inf_value,
                                                         unsigned batch, int nsteps, int thin, double* __restrict__ X_rec,
                                                         double* __restrict__ y_rec, double* __restrict__ X_last,
                                                         double* __restrict__ y_last, int64_t* __restrict__ naccept,
                                                         int64_t* __restrict__ ncalls, double* __restrict__ X_prop,
                                                         double* __restrict__ y_prop) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_L[GPRY_MAX_DIM * GPRY_MAX_DIM];
    __shared__ double s_x[GPRY_MAX_DIM], s_u[GPRY_MAX_DIM], s_z[GPRY_MAX_DIM];
    __shared__ double s_xt[GPRY_MAX_DIM], s_ut[GPRY_MAX_DIM];
    __shared__ double s_y;
    const int t = threadIdx.x, d = kp.d;
    const unsigned c = blockIdx.x;
    const int nrec = nsteps / thin;
    for (int e = t; e < d * d; e += 256) s_L[e] = Lp[e];
    if (t < d) {
        s_x[t] = X0[(int64_t)c * d + t];
        s_u[t] = (s_x[t] - a.lo[t]) / (a.hi[t] - a.lo[t]);
    }
    __syncthreads();
    int64_t n_eval = 0, n_acc = 0;
    double y_cur = y0[c];
    if (y_cur != y_cur) {                       // NaN: the start's y is evaluated here
        y_cur = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);
        n_eval++;
    }
    for (int s = 0; s < nsteps; s++) {
        if (t < (d + 1) / 2) ns_box_muller(s_z, t, d, ns_philox(a.seed, MC_PHASE, (unsigned)t, batch, c, (unsigned)s));
        __syncthreads();
        if (t < d) {
            double v = 0.0;
            for (int k = 0; k <= t; k++) v = v + ns_rn(s_L[t * d + k] * s_z[k]);
            const double u = s_u[t] + v;
            s_ut[t] = u;
            s_xt[t] = a.lo[t] + ns_rn(u * (a.hi[t] - a.lo[t]));
        }
        __syncthreads();
        bool inside = true;
        for (int k = 0; k < d; k++)
            inside = inside && s_ut[k] >= 0.0 && s_ut[k] <= 1.0 && s_xt[k] >= a.lo[k] && s_xt[k] <= a.hi[k];
        double yp = NAN;
        bool acc = false;
        if (inside) {
            yp = ns_eval<DP, KID>(s_xt, a, kp, ap, r2s, red, &s_y);
            n_eval++;
            const double ua = ns_philox(a.seed, MC_PHASE, MC_DRAW_ACCEPT, batch, c, (unsigned)s).a;
            acc = isfinite(yp) && yp > minus_inf_value && log(1.0 - ua) < (yp - y_cur) / T;
        }
        if (X_prop) {
            const int64_t p = (int64_t)c * nsteps + s;
            if (t < d) X_prop[p * d + t] = s_xt[t];
            if (t == 0) y_prop[p] = yp;
        }
        __syncthreads();                        // (every thread has read s_ut / s_xt)
        if (acc) {
            if (t < d) { s_x[t] = s_xt[t]; s_u[t] = s_ut[t]; }
            y_cur = yp;
            n_acc++;
        }
        __syncthreads();
        if ((s + 1) % thin == 0) {
            const int64_t r = (int64_t)c * nrec + (s + 1) / thin - 1;
            if (t < d) X_rec[r * d + t] = s_x[t];
            if (t == 0) y_rec[r] = y_cur;
        }
    }
    if (t < d) X_last[(int64_t)c * d + t] = s_x[t];
    if (t == 0) { y_last[c] = y_cur; naccept[c] = n_acc; ncalls[c] = n_eval; }
}

extern "C" {

int gpry_mcmc_chains(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                     int64_t nchains, const double* Lp, double T, double minus_inf_value, uint64_t seed, int64_t batch,
                     int nsteps, int thin, double* X_rec, double* y_rec, double* X_last, double* y_last,
                     int64_t* naccept, int64_t* ncalls, double* X_prop, double* y_prop, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_mcmc_chains: ctx is NULL");
    if (!lo || !hi || !X0 || !y0 || !Lp || !X_last || !y_last || !naccept || !ncalls)
        return gpry_fail(ctx, -1, "gpry_mcmc_chains: NULL argument");
    GPRY_TRY(ns_check_chains(ctx, "gpry_mcmc_chains", nchains, 0, nsteps, thin, batch, &T, X_rec, y_rec, X_prop, y_prop));
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_mcmc_chains", lo, hi, seed, &a, &kp, &ap));
    const int d = ctx->d;
    const int64_t n = nchains, nrec = nsteps / thin;
    NsStage st(ctx, ctx->opt_mcmc_mapped != 0);
    const auto rX0 = st.in(X0, n * d), ry0 = st.in(y0, n), rL = st.in(Lp, (int64_t)d * d);
    const auto rXr = st.out(X_rec, n * nrec * d), ryr = st.out(y_rec, n * nrec);
    const auto rXl = st.out(X_last, n * d), ryl = st.out(y_last, n);
    const auto rna = st.out(naccept, n), rnc = st.out(ncalls, n);
    const auto rXp = st.out(X_prop, n * nsteps * d), ryp = st.out(y_prop, n * nsteps);
    GPRY_TRY(st.begin());
#define MC(DP, KID) hipLaunchKernelGGL((mcmc_chain_kernel<DP, KID>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, \
                                       ap, st.dev(rX0), st.dev(ry0), st.dev(rL), T, minus_inf_value, (unsigned)batch,     \
                                       nsteps, thin, st.dev(rXr), st.dev(ryr), st.dev(rXl), st.dev(ryl), st.dev(rna),     \
                                       st.dev(rnc), st.dev(rXp), st.dev(ryp))
    DISPATCH_DP_KID(d, ctx->kernel_id, MC)
#undef MC
    return st.end(device_ms);
}

}  // extern "C"
