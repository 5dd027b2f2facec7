// Hamiltonian Monte Carlo of the surrogate's posterior mean on the device: the kernel behind gpry_hmc_chains and
// gpry_hmc_chains_reflect.  The adaptation of the mass matrix, of the step size and of the trajectory length, the
// convergence test (R - 1 over split chains), the burn-in and the temperature weights are host-side, in gpry_amd/hmc.py; together they stand in for the
// Cobaya MCMC runs of gpry/mc.py:173-327 (the surrogate's final sample), gpry/convergence.py:430-476 (GaussianKL's MC
// fallback) and gpry/proposal.py:359-443 (SmallChainProposer), as the Metropolis chains of mcmc.hip do.
//
// Likelihood.  ns_eval of ns_common.h at the end point of a trajectory: gpr.predict(x[None]) bit for bit, clip and gates
// included.  Gradient.  mean_grad of mean_grad.h: the gradient of the unclipped, ungated mean, taken to unit-cube
// coordinates: g_k = y_std (hi_k - lo_k) / span_k * mean_grad_k, span the model's own x-affine map (1 without one).  The
// gradient ignores clip and gates and only the acceptance sees them: any gradient field gives a reversible,
// volume-preserving leapfrog map, so the chain stays exact.
//
// Randomness.  ns_philox with phase 4: trajectory s of chain c in call `batch` takes the counters (4, draw j, batch, c,
// s); draws 0..15 give z ~ N(0, I) by Box-Muller (ns_box_muller), draw 16 the acceptance uniform ua, draw 17 the
// step-size jitter u: eps_s = eps (0.8 + 0.4 u).  No value depends on how many chains share a launch.
//
// Chains.  One 256-thread workgroup per chain, `nsteps` trajectories inside the kernel.  Coordinates are the unit cube's,
// u = (x - lo) / (hi - lo); the target is exp(y / T).  With momentum p = z (unit mass; Lp, lower triangular, is the
// factor of the inverse mass matrix): a half kick p += (eps_s / 2) Lp^T g(u) / T, then nleap times a drift
// u += eps_s Lp p and a kick (a full one, the last a half one).  A drift that leaves [0, 1]^d (the test of
// mcmc_chain_kernel) or a gradient that is not finite rejects the trajectory at once: nothing further is evaluated.
// (Leapfrog followed by a momentum flip is an involution, and the set of states whose whole trajectory stays inside the
// box is invariant under it.)  Otherwise y' = ns_eval(x') and the trajectory is accepted iff y' is finite,
// y' > minus_inf_value and log(1 - ua) < (y' - y) / T - (|p'|^2 - |p|^2) / 2.  The gradient at the current state is
// kept between trajectories: a trajectory costs nleap gradients and one mean.  Every product that feeds a sum goes
// through ns_rn, so that no FMA fuses them (-ffp-contract=fast) and the host can restate the trajectory.
//
// Reflection (RF, gpry_hmc_chains_reflect with reflect set).  The drift becomes a billiard flow of duration tau = eps_s
// inside [0, 1]^d.  Repeat: the velocity v = Lp p (the sum of the plain drift, in its order); the hit time of every
// coordinate's wall, t_k = ((v_k > 0 ? 1 : 0) - u_k) / v_k (+inf for v_k = 0), and j, the lowest index with the smallest;
// without a hit before tau, u += rn(tau v) and the drift is done -- a drift that never hits is the plain drift bit for bit.
// Otherwise u_t += rn(t_j v_t) (t != j), u_j is set on its wall exactly, p is reflected about the wall's normal in the
// whitened coordinates, r = row j of Lp: p_k -= rn((rn(2 a) / b) r_k), a = sum rn(r_k p_k) (= v_j), b = sum rn(r_k r_k),
// k <= j, and tau -= t_j.  u is clamped to [0, 1] after every move and x to [lo, hi] after the drift, which acts at
// rounding level only, so the box test below never fires on an overshoot.  A drift that would need more than max_reflect
// reflections rejects the trajectory unevaluated, as a box exit does without RF.  (In q = Lp^-1 u the flow is free motion
// with specular reflection at the planes r . q = const: volume-preserving and time-reversible, and a reflection keeps
// |p|^2; so leapfrog with this drift followed by a momentum flip is still an involution, and the set of states whose
// trajectory stays within the cap in every drift is invariant under it, the reversed trajectory meeting the same walls.)
// No draw is added, and the kicks, the gradient, the acceptance rule and the records are those of the plain kernel.
#include "ns_common.h"
#include "mean_grad.h"

#define HMC_PHASE 4u
#define HMC_DRAW_ACCEPT 16u         // draws 0..15 of a trajectory: z; 16: the acceptance uniform; 17: the step-size jitter
#define HMC_DRAW_JITTER 17u

// |p|^2 with the products rounded, in the order of the coordinates (every thread: p is in LDS)
__device__ __forceinline__ double hmc_norm2(const double* p, int d) {
    double v = 0.0;
    for (int k = 0; k < d; k++) v = v + ns_rn(p[k] * p[k]);
    return v;
}

// Outputs, per chain c: as mcmc_chain_kernel's, and ngrad, the gradient evaluations.  Test hooks (each nullable):
// X_prop / y_prop, the last point of every trajectory (where it ended, or where it was cut short) and its y, NaN where it
// was not evaluated; dH_prop, the right-hand side of the acceptance test (NaN likewise); G0, g at the start state.
// RF: rf.max_reflect, and rf.nreflect (nullable), the reflections of the chain; without RF the argument is empty, so
// that the plain kernels keep the code they had before there was a flag.
template <bool RF> struct HmcRf { int max_reflect; int64_t* nreflect; };
template <> struct HmcRf<false> {};

template <int DP, int KID, bool RF>
__global__ __launch_bounds__(256) void hmc_chain_kernel(NsArgs a, KernParams kp, AffParams ap,
                                                        const double* __restrict__ X0, const double* __restrict__ y0,
                                                        const double* __restrict__ Lp, double eps, int nleap, double T,
                                                        double minus_inf_value, unsigned batch, int nsteps, int thin,
                                                        double* __restrict__ X_rec, double* __restrict__ y_rec,
                                                        double* __restrict__ X_last, double* __restrict__ y_last,
                                                        int64_t* __restrict__ naccept, int64_t* __restrict__ ncalls,
                                                        int64_t* __restrict__ ngrad, double* __restrict__ X_prop,
                                                        double* __restrict__ y_prop, double* __restrict__ dH_prop,
                                                        double* __restrict__ G0, HmcRf<RF> rf) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_L[GPRY_MAX_DIM * GPRY_MAX_DIM];
    __shared__ double s_gl[MEAN_GRAD_LDS];
    __shared__ double s_x[GPRY_MAX_DIM], s_u[GPRY_MAX_DIM], s_g[GPRY_MAX_DIM];
    __shared__ double s_xt[GPRY_MAX_DIM], s_ut[GPRY_MAX_DIM], s_gt[GPRY_MAX_DIM];
    __shared__ double s_p[GPRY_MAX_DIM], s_xs[GPRY_MAX_DIM], s_gs[GPRY_MAX_DIM];
    __shared__ double s_y;
    const int t = threadIdx.x, d = kp.d;
    const unsigned c = blockIdx.x;
    const int nrec = nsteps / thin;
    for (int e = t; e < d * d; e += 256) s_L[e] = Lp[e];
    if (t < GPRY_MAX_DIM) {
        s_xs[t] = 0.0;
        s_gs[t] = 0.0;
    }
    if (t < d) {
        s_x[t] = X0[(int64_t)c * d + t];
        s_u[t] = (s_x[t] - a.lo[t]) / (a.hi[t] - a.lo[t]);
        // d y / d u_k over the gradient of the transformed mean in the kernel's coordinates
        s_gs[t] = a.y_std * ((a.hi[t] - a.lo[t]) / (kp.has_aff ? ap.span[t] : 1.0));
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
    int64_t n_eval = 0, n_acc = 0, n_grad = 0, n_refl = 0;
    double y_cur = y0[c];
    if (y_cur != y_cur) {                       // NaN: the start's y is evaluated here
        y_cur = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);
        n_eval++;
    }
    grad_at(s_x, s_g);
    n_grad++;
    if (G0 && t < d) G0[(int64_t)c * d + t] = s_g[t];
    for (int s = 0; s < nsteps; s++) {
        if (t < (d + 1) / 2) ns_box_muller(s_p, t, d, ns_philox(a.seed, HMC_PHASE, (unsigned)t, batch, c, (unsigned)s));
        if (t < d) { s_ut[t] = s_u[t]; s_xt[t] = s_x[t]; s_gt[t] = s_g[t]; }
        __syncthreads();
        const double uj = ns_philox(a.seed, HMC_PHASE, HMC_DRAW_JITTER, batch, c, (unsigned)s).a;
        const double eps_s = ns_rn(eps * (0.8 + ns_rn(0.4 * uj)));
        const double k_full = eps_s / T, k_half = ns_rn(0.5 * eps_s) / T;
        const double K0 = hmc_norm2(s_p, d);
        bool alive = true;
        for (int k = 0; k < d; k++) alive = alive && isfinite(s_gt[k]);
        __syncthreads();                        // (every thread has read s_p before the kick writes it)
        for (int l = 0; l <= nleap && alive; l++) {
            // kick with the gradient at the trial point: p += c Lp^T g
            if (t < d) {
                double v = 0.0;
                for (int i = t; i < d; i++) v = v + ns_rn(s_L[i * d + t] * s_gt[i]);
                s_p[t] = s_p[t] + ns_rn(((l == 0 || l == nleap) ? k_half : k_full) * v);
            }
            __syncthreads();
            if (l == nleap) break;
            // drift: u += eps_s Lp p
            double un = 0.0, xn = 0.0;
            if constexpr (RF) {
                // the billiard flow of duration eps_s: j, tj, tau and nr are the same in every thread
                __shared__ double s_v[GPRY_MAX_DIM], s_th[GPRY_MAX_DIM];        // velocity and hit times
                double tau = eps_s;
                for (int nr = 0;; nr++) {
                    double v = 0.0;
                    if (t < d) {
                        for (int k = 0; k <= t; k++) v = v + ns_rn(s_L[t * d + k] * s_p[k]);
                        s_v[t] = v;
                        s_th[t] = v != 0.0 ? ((v > 0.0 ? 1.0 : 0.0) - s_ut[t]) / v : INFINITY;
                    }
                    __syncthreads();
                    int j = -1;
                    double tj = INFINITY;
                    for (int k = 0; k < d; k++)
                        if (s_th[k] < tj) { tj = s_th[k]; j = k; }
                    if (!(tj < tau)) {              // no wall within what is left: the plain move ends the drift
                        if (t < d) un = s_ut[t] + ns_rn(tau * v);
                        break;
                    }
                    if (nr == rf.max_reflect) {        // the cap: the trajectory ends where it is
                        alive = false;
                        if (t < d) un = s_ut[t];
                        break;
                    }
                    if (t < d) un = t == j ? (s_v[j] > 0.0 ? 1.0 : 0.0) : s_ut[t] + ns_rn(tj * v);
                    if (t < d) s_ut[t] = un < 0.0 ? 0.0 : (un > 1.0 ? 1.0 : un);
                    if (t <= j) {                   // p -= (2 a / b) r, r = row j of Lp, a = r . p = v_j
                        const double* r = s_L + j * d;
                        double b = 0.0;
                        for (int k = 0; k <= j; k++) b = b + ns_rn(r[k] * r[k]);
                        s_p[t] = s_p[t] - ns_rn((ns_rn(2.0 * s_v[j]) / b) * r[t]);
                    }
                    tau = tau - tj;
                    n_refl++;
                    __syncthreads();                // (s_p, s_ut written; s_v, s_th read)
                }
                if (t < d) {
                    un = un < 0.0 ? 0.0 : (un > 1.0 ? 1.0 : un);
                    xn = a.lo[t] + ns_rn(un * (a.hi[t] - a.lo[t]));
                    xn = xn < a.lo[t] ? a.lo[t] : (xn > a.hi[t] ? a.hi[t] : xn);
                }
            } else if (t < d) {
                double v = 0.0;
                for (int k = 0; k <= t; k++) v = v + ns_rn(s_L[t * d + k] * s_p[k]);
                un = s_ut[t] + ns_rn(eps_s * v);
                xn = a.lo[t] + ns_rn(un * (a.hi[t] - a.lo[t]));
            }
            if (t < d) { s_ut[t] = un; s_xt[t] = xn; }
            __syncthreads();
            for (int k = 0; k < d; k++)
                alive = alive && s_ut[k] >= 0.0 && s_ut[k] <= 1.0 && s_xt[k] >= a.lo[k] && s_xt[k] <= a.hi[k];
            if (!alive) break;
            grad_at(s_xt, s_gt);
            n_grad++;
            for (int k = 0; k < d; k++) alive = alive && isfinite(s_gt[k]);
        }
        double yp = NAN, dH = NAN;
        bool acc = false;
        if (alive) {
            yp = ns_eval<DP, KID>(s_xt, a, kp, ap, r2s, red, &s_y);
            n_eval++;
            const double ua = ns_philox(a.seed, HMC_PHASE, HMC_DRAW_ACCEPT, batch, c, (unsigned)s).a;
            dH = (yp - y_cur) / T - ns_rn(0.5 * (hmc_norm2(s_p, d) - K0));
            acc = isfinite(yp) && yp > minus_inf_value && log(1.0 - ua) < dH;
        }
        if (X_prop) {
            const int64_t p = (int64_t)c * nsteps + s;
            if (t < d) X_prop[p * d + t] = s_xt[t];
            if (t == 0) y_prop[p] = yp;
        }
        if (dH_prop && t == 0) dH_prop[(int64_t)c * nsteps + s] = dH;
        __syncthreads();                        // (every thread has read s_p / s_ut / s_xt / s_gt)
        if (acc) {
            if (t < d) { s_x[t] = s_xt[t]; s_u[t] = s_ut[t]; s_g[t] = s_gt[t]; }
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
    if (t == 0) { y_last[c] = y_cur; naccept[c] = n_acc; ncalls[c] = n_eval; ngrad[c] = n_grad; }
    if constexpr (RF)
        if (rf.nreflect && t == 0) rf.nreflect[c] = n_refl;
}

extern "C" {

int gpry_hmc_chains_reflect(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                            int64_t nchains, const double* Lp, double eps, int nleap, double T, double minus_inf_value,
                            uint64_t seed, int64_t batch, int nsteps, int thin, double* X_rec, double* y_rec,
                            double* X_last, double* y_last, int64_t* naccept, int64_t* ncalls, int64_t* ngrad,
                            double* X_prop, double* y_prop, double* dH_prop, double* G0, int reflect, int max_reflect,
                            int64_t* nreflect, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_hmc_chains: ctx is NULL");
    if (!lo || !hi || !X0 || !y0 || !Lp || !X_last || !y_last || !naccept || !ncalls || !ngrad)
        return gpry_fail(ctx, -1, "gpry_hmc_chains: NULL argument");
    GPRY_TRY(ns_check_chains(ctx, "gpry_hmc_chains", nchains, 0, nsteps, thin, batch, &T, X_rec, y_rec, X_prop, y_prop));
    if (!(eps > 0.0) || !isfinite(eps)) return gpry_fail(ctx, -1, "gpry_hmc_chains: step size eps = %g", eps);
    if (nleap < 1 || nleap > 1024) return gpry_fail(ctx, -1, "gpry_hmc_chains: nleap = %d is outside 1 .. 1024", nleap);
    if (reflect && (max_reflect < 1 || max_reflect > 1024))
        return gpry_fail(ctx, -1, "gpry_hmc_chains: max_reflect = %d is outside 1 .. 1024", max_reflect);
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_hmc_chains", lo, hi, seed, &a, &kp, &ap));
    const int d = ctx->d;
    const int64_t n = nchains, nrec = nsteps / thin;
    NsStage st(ctx);
    const auto rX0 = st.in(X0, n * d), ry0 = st.in(y0, n), rL = st.in(Lp, (int64_t)d * d);
    const auto rXr = st.out(X_rec, n * nrec * d), ryr = st.out(y_rec, n * nrec);
    const auto rXl = st.out(X_last, n * d), ryl = st.out(y_last, n);
    const auto rna = st.out(naccept, n), rnc = st.out(ncalls, n), rgr = st.out(ngrad, n);
    const auto rXp = st.out(X_prop, n * nsteps * d), ryp = st.out(y_prop, n * nsteps), rdH = st.out(dH_prop, n * nsteps);
    const auto rG0 = st.out(G0, n * d);
    const auto rnr = st.out(reflect ? nreflect : nullptr, n);
    GPRY_TRY(st.begin());
#define HM(DP, KID, RF, RFARG)                                                                                           \
    hipLaunchKernelGGL((hmc_chain_kernel<DP, KID, RF>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap,          \
                       st.dev(rX0), st.dev(ry0), st.dev(rL), eps, nleap, T, minus_inf_value, (unsigned)batch, nsteps, thin,  \
                       st.dev(rXr), st.dev(ryr), st.dev(rXl), st.dev(ryl), st.dev(rna), st.dev(rnc), st.dev(rgr),          \
                       st.dev(rXp), st.dev(ryp), st.dev(rdH), st.dev(rG0), RFARG)
#define HM_PLAIN(DP, KID) HM(DP, KID, false, HmcRf<false>{})
#define HM_RF(DP, KID) HM(DP, KID, true, (HmcRf<true>{max_reflect, st.dev(rnr)}))
    if (reflect) { DISPATCH_DP_KID(d, ctx->kernel_id, HM_RF) }
    else { DISPATCH_DP_KID(d, ctx->kernel_id, HM_PLAIN) }
#undef HM_RF
#undef HM_PLAIN
#undef HM
    if (!reflect && nreflect) memset(nreflect, 0, 8 * n);
    return st.end(device_ms);
}

int gpry_hmc_chains(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0, int64_t nchains,
                    const double* Lp, double eps, int nleap, double T, double minus_inf_value, uint64_t seed,
                    int64_t batch, int nsteps, int thin, double* X_rec, double* y_rec, double* X_last, double* y_last,
                    int64_t* naccept, int64_t* ncalls, int64_t* ngrad, double* X_prop, double* y_prop, double* dH_prop,
                    double* G0, double* device_ms) {
    return gpry_hmc_chains_reflect(ctx, lo, hi, X0, y0, nchains, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps,
                                   thin, X_rec, y_rec, X_last, y_last, naccept, ncalls, ngrad, X_prop, y_prop, dH_prop, G0, 0,
                                   0, nullptr, device_ms);
}

}  // extern "C"
