// Tempered Metropolis ladders of the surrogate's posterior mean on the device: the kernel behind gpry_mcmc_ladders.
// The ladder's construction, the adaptation, R - 1 over the cold rungs and the weights are host-side, in
// gpry_amd/tempering.py.
//
// One 256-thread workgroup is one ladder of `nrungs` <= RP chains; slot r of ladder a is chain c = a nrungs + r and makes
// the Metropolis step of mcmc_chain_kernel (mcmc.hip) for chain c with its own proposal factor Lp[r] and temperature
// T[r]: the same Philox counters (3, j, batch, c, s), j = 0..15 for z and 16 for ua, the same ns_rn fences, box test and
// acceptance rule.  What differs is how the work is laid out: thread t serves coordinate t % 32 of slot t / 32, all slots
// propose at the same time, and the proposals inside the box are evaluated together by ns_eval_multi (ns_common.h) --
// one pass over the training rows, each row and each alpha loaded once and used for every slot, every y with the bits of
// gpry_predict of its point alone.  With swap_every = 0 slot r is chain c of gpry_mcmc_chains, bit for bit.
//
// Swap rounds.  After step s with (s + 1) % swap_every == 0, round q = (s + 1) / swap_every - 1 tries the pairs (r, r + 1)
// with r = q (mod 2): iff both current y are finite and above minus_inf_value, with us = draw 17 of the counters of chain
// c_r at step s, the pair exchanges (x, u, y) iff log(1 - us) < (1 / T[r] - 1 / T[r + 1]) (y_{r+1} - y_r).  Temperatures
// and proposals stay with the slot.  Everything happens inside the workgroup: no atomics, no traffic between workgroups
// and no waiting; every barrier is reached under conditions that are the same for the whole workgroup (the step number,
// the mask of slots to evaluate).
#include "ns_common.h"

#define ML_PHASE 3u
#define ML_DRAW_ACCEPT 16u
#define ML_DRAW_SWAP 17u
#define ML_MAX_RUNGS 8

// bit p set iff `ok` holds in all 32 threads of slot p: one ballot per wave (a wave holds two slots), the verdicts
// through LDS.  The barrier inside also orders what the threads wrote to LDS before the call.
template <int RP>
__device__ __forceinline__ unsigned ml_slot_mask(bool ok, int* s_flag) {
    const int t = threadIdx.x;
    const unsigned long long b = __ballot(ok);
    if ((t & 31) == 0 && (t >> 5) < RP) s_flag[t >> 5] = (unsigned)(b >> (t & 32)) == 0xffffffffu;
    __syncthreads();
    unsigned mask = 0;
#pragma unroll
    for (int p = 0; p < RP; p++) mask |= s_flag[p] ? 1u << p : 0u;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)mask);
}

template <int RP>
__device__ __forceinline__ double ml_pick(const double (&y)[RP], int p) {
    double v = NAN;
#pragma unroll
    for (int q = 0; q < RP; q++) v = q == p ? y[q] : v;
    return v;
}

// Outputs per chain c as those of mcmc_chain_kernel; per ladder and adjacent pair the tried and accepted swaps.  Test
// hooks: X_prop / y_prop as in mcmc_chain_kernel; swap_log (nladders x nsteps / swap_every x (nrungs - 1)): 1 accepted,
// 0 tried and rejected, -1 not tried (the other parity's pairs included).
template <int DP, int KID, int RP>
__global__ __launch_bounds__(256) void ladder_chain_kernel(NsArgs a, KernParams kp, AffParams ap, int nrungs,
                                                           const double* __restrict__ X0, const double* __restrict__ y0,
                                                           const double* __restrict__ Lp, const double* __restrict__ T,
                                                           double minus_inf_value, unsigned batch, int nsteps, int thin,
                                                           int swap_every, double* __restrict__ X_rec,
                                                           double* __restrict__ y_rec, double* __restrict__ X_last,
                                                           double* __restrict__ y_last, int64_t* __restrict__ naccept,
                                                           int64_t* __restrict__ ncalls, int64_t* __restrict__ nswap_try,
                                                           int64_t* __restrict__ nswap_acc, double* __restrict__ X_prop,
                                                           double* __restrict__ y_prop, int8_t* __restrict__ swap_log) {
    static_assert(GPRY_MAX_DIM == 32 && RP <= ML_MAX_RUNGS, "thread t serves coordinate t % 32 of slot t / 32");
    __shared__ double r2s[RP * MEAN_MULTI_CH];
    __shared__ double s_x[RP * GPRY_MAX_DIM], s_u[RP * GPRY_MAX_DIM], s_z[RP * GPRY_MAX_DIM];
    __shared__ double s_xt[RP * GPRY_MAX_DIM], s_ut[RP * GPRY_MAX_DIM];
    __shared__ double s_y[RP], s_yc[RP], s_T[RP];
    __shared__ int s_flag[RP];
    const int t = threadIdx.x, d = kp.d;
    const int p = t >> 5, k = t & 31, e = t;                // slot, coordinate, and this thread's place in the s_* arrays
    const bool live = p < nrungs;                           // (surplus slots are masked out for good)
    const bool mine = live && k < d;
    const int64_t ladder = blockIdx.x;
    const unsigned c = (unsigned)(ladder * nrungs + (live ? p : 0));
    const int nrec = nsteps / thin;
    const double* L = Lp + (int64_t)(live ? p : 0) * d * d;
    double Tp = 1.0, y_cur = 0.0;
    if (live) {
        Tp = T[p];
        y_cur = y0[c];
        if (k == 0) s_T[p] = Tp;
    }
    if (mine) {
        s_x[e] = X0[(int64_t)c * d + k];
        s_u[e] = (s_x[e] - a.lo[k]) / (a.hi[k] - a.lo[k]);
        s_xt[e] = s_x[e];
    }
    int64_t n_eval = 0, n_acc = 0, n_try = 0, n_sacc = 0;
    double yv[RP];
#pragma unroll
    for (int q = 0; q < RP; q++) yv[q] = NAN;
    // pass -1 evaluates the starts whose y0 is NaN (s_xt holds them), passes 0 .. nsteps - 1 are the steps: ONE call
    // of ns_eval_multi serves both
    for (int s = -1; s < nsteps; s++) {
        bool ok = live && y_cur != y_cur;
        if (s >= 0) {
            if (live && k < (d + 1) / 2)
                ns_box_muller(s_z + p * GPRY_MAX_DIM, k, d, ns_philox(a.seed, ML_PHASE, (unsigned)k, batch, c, (unsigned)s));
            __syncthreads();
            ok = live;
            if (mine) {
                double v = 0.0;
                for (int j = 0; j <= k; j++) v = v + ns_rn(L[k * d + j] * s_z[p * GPRY_MAX_DIM + j]);
                const double u = s_u[e] + v;
                const double xt = a.lo[k] + ns_rn(u * (a.hi[k] - a.lo[k]));
                s_ut[e] = u;
                s_xt[e] = xt;
                ok = u >= 0.0 && u <= 1.0 && xt >= a.lo[k] && xt <= a.hi[k];
            }
        }
        const unsigned inside = ml_slot_mask<RP>(ok, s_flag);
        ns_eval_multi<DP, KID, RP>(s_xt, inside, a, kp, ap, r2s, s_y, yv);
        if (s < 0) {
            if (ok) { y_cur = ml_pick<RP>(yv, p); n_eval++; }
            continue;
        }
        double yp = NAN;
        bool acc = false;
        if (live && (inside >> p & 1u)) {
            yp = ml_pick<RP>(yv, p);
            n_eval++;
            const double ua = ns_philox(a.seed, ML_PHASE, ML_DRAW_ACCEPT, batch, c, (unsigned)s).a;
            acc = isfinite(yp) && yp > minus_inf_value && log(1.0 - ua) < (yp - y_cur) / Tp;
        }
        if (X_prop && live) {
            const int64_t i = (int64_t)c * nsteps + s;
            if (k < d) X_prop[i * d + k] = s_xt[e];
            if (k == 0) y_prop[i] = yp;
        }
        if (acc) {                                          // (s_x / s_u at e are this thread's own)
            if (k < d) { s_x[e] = s_xt[e]; s_u[e] = s_ut[e]; }
            y_cur = yp;
            n_acc++;
        }
        if (swap_every > 0 && (s + 1) % swap_every == 0) {
            const int q = (s + 1) / swap_every - 1;
            if (live && k == 0) s_yc[p] = y_cur;
            __syncthreads();
            // the pair of this slot in round q: (r, r + 1), r = q (mod 2); both of its slots take the same decision
            const int r = ((p ^ q) & 1) ? p - 1 : p;
            const bool paired = live && r >= 0 && r + 1 < nrungs;
            bool tried = false, swapped = false;
            double ylo = 0.0, yhi = 0.0;
            if (paired) {
                ylo = s_yc[r]; yhi = s_yc[r + 1];
                tried = isfinite(ylo) && ylo > minus_inf_value && isfinite(yhi) && yhi > minus_inf_value;
                if (tried) {
                    const double us = ns_philox(a.seed, ML_PHASE, ML_DRAW_SWAP, batch, (unsigned)(ladder * nrungs + r),
                                                (unsigned)s).a;
                    swapped = log(1.0 - us) < (1.0 / s_T[r] - 1.0 / s_T[r + 1]) * (yhi - ylo);
                }
            }
            const int o = (p == r ? p + 1 : p - 1) * GPRY_MAX_DIM + k;      // the other slot's place
            double ox = 0.0, ou = 0.0;
            if (swapped && k < d) { ox = s_x[o]; ou = s_u[o]; }
            __syncthreads();
            if (swapped) {
                if (k < d) { s_x[e] = ox; s_u[e] = ou; }
                y_cur = p == r ? yhi : ylo;
            }
            if (live && k == 0 && p + 1 < nrungs) {         // slot p keeps the books of the pair (p, p + 1)
                const bool here = p == r;
                n_try += here && tried;
                n_sacc += here && swapped;
                if (swap_log)
                    swap_log[(ladder * (nsteps / swap_every) + q) * (nrungs - 1) + p] =
                        (here && tried) ? (swapped ? 1 : 0) : -1;
            }
        }
        if ((s + 1) % thin == 0 && live) {
            const int64_t i = (int64_t)c * nrec + (s + 1) / thin - 1;
            if (k < d) X_rec[i * d + k] = s_x[e];
            if (k == 0) y_rec[i] = y_cur;
        }
    }
    if (mine) X_last[(int64_t)c * d + k] = s_x[e];
    if (live && k == 0) {
        y_last[c] = y_cur; naccept[c] = n_acc; ncalls[c] = n_eval;
        if (p + 1 < nrungs) {
            nswap_try[ladder * (nrungs - 1) + p] = n_try;
            nswap_acc[ladder * (nrungs - 1) + p] = n_sacc;
        }
    }
}

extern "C" {

int gpry_mcmc_ladders(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                      int64_t nladders, int nrungs, const double* Lp, const double* T, double minus_inf_value,
                      uint64_t seed, int64_t batch, int nsteps, int thin, int swap_every, double* X_rec, double* y_rec,
                      double* X_last, double* y_last, int64_t* naccept, int64_t* ncalls, int64_t* nswap_try,
                      int64_t* nswap_acc, double* X_prop, double* y_prop, int8_t* swap_log, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_mcmc_ladders: ctx is NULL");
    if (!lo || !hi || !X0 || !y0 || !Lp || !T || !X_last || !y_last || !naccept || !ncalls)
        return gpry_fail(ctx, -1, "gpry_mcmc_ladders: NULL argument");
    if (nrungs < 1 || nrungs > ML_MAX_RUNGS)
        return gpry_fail(ctx, -1, "gpry_mcmc_ladders: nrungs = %d outside 1 .. %d", nrungs, ML_MAX_RUNGS);
    GPRY_TRY(ns_check_chains(ctx, "gpry_mcmc_ladders", nladders, nrungs, nsteps, thin, batch, T, X_rec, y_rec, X_prop, y_prop));
    if (swap_every < 0) return gpry_fail(ctx, -1, "gpry_mcmc_ladders: swap_every = %d", swap_every);
    if (swap_log && swap_every == 0)
        return gpry_fail(ctx, -1, "gpry_mcmc_ladders: swap_log given with swap_every = 0");
    if (nrungs > 1 && (!nswap_try || !nswap_acc)) return gpry_fail(ctx, -1, "gpry_mcmc_ladders: NULL argument");
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "gpry_mcmc_ladders", lo, hi, seed, &a, &kp, &ap));
    const int d = ctx->d;
    const int64_t n = nladders * nrungs, npair = nladders * (nrungs - 1), nrec = nsteps / thin;
    const int64_t nround = swap_every > 0 ? nsteps / swap_every : 0;
    NsStage st(ctx, ctx->opt_mcmc_mapped != 0);
    const auto rX0 = st.in(X0, n * d), ry0 = st.in(y0, n), rL = st.in(Lp, (int64_t)nrungs * d * d), rT = st.in(T, nrungs);
    const auto rXr = st.out(X_rec, n * nrec * d), ryr = st.out(y_rec, n * nrec);
    const auto rXl = st.out(X_last, n * d), ryl = st.out(y_last, n);
    const auto rna = st.out(naccept, n), rnc = st.out(ncalls, n);
    const auto rst = st.out(nswap_try, npair), rsa = st.out(nswap_acc, npair);
    const auto rXp = st.out(X_prop, n * nsteps * d), ryp = st.out(y_prop, n * nsteps);
    const auto rsl = st.out(swap_log, nround * npair);
    GPRY_TRY(st.begin());
#define ML_(DP, KID, RP) hipLaunchKernelGGL((ladder_chain_kernel<DP, KID, RP>), dim3((unsigned)nladders), dim3(256), 0,      \
                                            ctx->stream, a, kp, ap, nrungs, st.dev(rX0), st.dev(ry0), st.dev(rL), st.dev(rT), \
                                            minus_inf_value, (unsigned)batch, nsteps, thin, swap_every, st.dev(rXr),          \
                                            st.dev(ryr), st.dev(rXl), st.dev(ryl), st.dev(rna), st.dev(rnc), st.dev(rst),     \
                                            st.dev(rsa), st.dev(rXp), st.dev(ryp), st.dev(rsl))
    // RP: the smallest of 2 / 4 / 8 that holds the ladder
#define ML(DP, KID) if (nrungs <= 2) { ML_(DP, KID, 2); } else if (nrungs <= 4) { ML_(DP, KID, 4); } else { ML_(DP, KID, 8); }
    DISPATCH_DP_KID(d, ctx->kernel_id, ML)
#undef ML
#undef ML_
    return st.end(device_ms);
}

}  // extern "C"
