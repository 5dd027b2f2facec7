// Nested sampling of the surrogate's posterior mean on the device: the two kernels behind gpry_ns_prior and
// gpry_ns_generation.  The bookkeeping (sorting, prior volumes, whitening matrix, stopping, weights, evidence) is
// host-side, in gpry_amd/nested.py; it replaces the PolyChord / UltraNest runs of gpry/gp_acquisition.py:760-856,
// which call gpr.predict once per point.
//
// Likelihood.  y(x) is gpr.predict(x[None]) bit for bit: the slices of the one-point path (nsplit = clamp(N / 1024, 1, 8),
// the same rows_per_split, mean_slice of kern_math.h), added in slice order from 0.0; then fmin(mu * y_std + y_mean,
// clip_hi) written with explicit roundings (the library builds with -ffp-contract=fast, which would fuse it into an FMA
// on the device while the host computes a product and a sum -- and __dmul_rn / __dadd_rn are plain operators in this
// toolchain's headers, which it contracts all the same: ns_rn() hides the product from the combiner); then the gates of
// point_gate_bits (what the resident predict kernel applies), -inf for a gated point.
//
// Randomness.  Philox4x32-10 keyed by the seed; every draw has a fixed counter (phase, generation, chain, step, draw)
// -- word 0 = phase << 24 | draw, 1 = generation, 2 = chain (the point's index in the prior phase), 3 = step -- so no
// value depends on how workgroups are scheduled.  tests/tools/ns_philox.py restates it in numpy.
//
// Chains.  One 256-thread workgroup per chain, the whole walk of `num_repeats` slice-sampling steps (Neal 2003:
// stepping out, then shrinkage) inside the kernel.  Chains never communicate; the host launches one kernel per
// generation.
//
// Clusters.  gpry_ns_knn tables the k nearest neighbours of every live point (unit-cube coordinates) for the host's
// clustering rule (nested.py: knn_clusters); gpry_ns_generation_clustered then gives every chain the whitening matrix
// of its starting survivor's cluster.  Without labels the chain kernel is the unclustered one, bit for bit.
// gpry_ns_generation_volumes lets every chain first draw its cluster from cumulative probabilities (the clusters' prior
// volumes, PolyChord's choice) and then its start among that cluster's survivors; without a member list the chain
// kernel draws its start uniformly from all survivors, as before, bit for bit.
//
// Phantoms.  gpry_ns_generation_phantoms also keeps the chains' interior states: the state after every thin-th step but
// the last goes to X_ph / y_ph (PolyChord's phantom points).  The recording is a template flag of the chain kernel: no
// draw, evaluation or barrier is added, and without it the kernel is the instantiation of before.
//
// Host side.  The four gpry_ns_generation* entry points fill in an NsGenRequest by name; ns_generation_impl checks it
// (ns_check), lays out one pinned buffer (ns_layout of ns_common.h over the NS_* regions), fills it (ns_members: the
// clusters' member lists), launches (ns_launch_chains) and copies back.
#include <climits>
#include <vector>

#include "ns_common.h"

#define NS_PHASE_PRIOR 0u
#define NS_PHASE_START 1u
#define NS_PHASE_STEP 2u
#define NS_STEP_OUT_MAX 32
#define NS_SHRINK_MAX 64
#define NS_DRAW_OFFSET 16u          // draws 0..15 of a step: the normal vector z (two coordinates per draw)
#define NS_DRAW_SHRINK 17u          // draws 17..17+63: the shrinkage tries
#define NS_KNN_MAX_K 32
#define NS_KNN_MAX_N 65536
#define NS_KNN_LDS_N 7680           // rows of up to this many points keep their distances in LDS (60 KiB + 3.3 KiB static)
#define NS_PHANTOM_MAX_BYTES (1ll << 30)    // X_ph and y_ph of one generation together (gpry_hip.h)

// Prior draws: point i (one workgroup) is lo + u * (hi - lo), u from the counter (PRIOR, draw j, 0, i, 0) for
// coordinates 2j and 2j + 1, clamped to hi.
template <int DP, int KID>
__global__ __launch_bounds__(256) void ns_prior_kernel(NsArgs a, KernParams kp, AffParams ap, double* __restrict__ X_out,
                                                       double* __restrict__ y_out) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_x[GPRY_MAX_DIM];
    __shared__ double s_y;
    const int t = threadIdx.x;
    const unsigned i = blockIdx.x;
    if (t < kp.d) {
        const NsU2 u = ns_philox(a.seed, NS_PHASE_PRIOR, (unsigned)(t / 2), 0u, i, 0u);
        const double span = a.hi[t] - a.lo[t];
        const double x = fmin(a.lo[t] + ns_rn(((t & 1) ? u.b : u.a) * span), a.hi[t]);
        s_x[t] = x;
        X_out[(int64_t)i * kp.d + t] = x;
    }
    __syncthreads();
    const double y = ns_eval<DP, KID>(s_x, a, kp, ap, r2s, red, &s_y);
    if (t == 0) y_out[i] = y;
}

// One generation: chain c starts from a survivor drawn uniformly (counter (START, 0, gen, c, 0)) and makes
// `num_repeats` slice-sampling steps on {x in the box : y(x) > lstar}.  Step s: direction v = W z / |z| (with labels: W of
// the start's cluster, W + labels[j] d d), z ~ N(0, I) from draws 0..(d-1)/2 (ns_box_muller); the interval [-r, 1 - r]
// along v (r: draw 16) stepped out by whole widths, at most 32 per side (a side that reaches 32 widths stops growing and
// the step goes on to shrink from the interval it has); then up to 64 shrinkage tries (draws 17..), each uniform on the
// interval, a failed try at t moving the end on t's side of the current point (t < 0: the left one).  A step whose 64
// tries all fail keeps the current point.  A try outside the box fails without an evaluation.  W is lower
// triangular: the sum over k stops at the row's index, what lies above the diagonal is never read.
// tests/tools/sampler_walk.py restates the walk step by step.  Outputs: the chain's last point, its y and the number of
// evaluations it made.
// With a member list (volumes): chain c first draws its cluster q, the first q with u1 < cum_p[q] (u1: counter
// (START, 1, gen, c, 0)), then its start members[moffs[q] + min(floor(u0 n_q), n_q - 1)] from the same u0 as above
// (n_q = moffs[q + 1] - moffs[q]), and walks with W + q d d.  The host guarantees cum_p[n_clusters - 1] = 1.0 and
// n_q >= 1 wherever cum_p rises.
// PH (phantoms): after step s with (s + 1) % thin == 0 and s + 1 < num_repeats the chain's state (s_x, y_cur) goes to slot
// (s + 1) / thin - 1 of its n_ph = (num_repeats - 1) / thin rows of X_ph / y_ph.  Thread t stores the s_x[t] it wrote itself
// and every thread holds y_cur, so the stores need no barrier of their own; a chain that did not move stores the same
// state again (a repeated sample).  Without PH the three arguments are not read.
template <int DP, int KID, bool PH>
__global__ __launch_bounds__(256) void ns_chain_kernel(NsArgs a, KernParams kp, AffParams ap,
                                                       const double* __restrict__ X_surv, const double* __restrict__ y_surv,
                                                       int64_t nsurv, const double* __restrict__ W,
                                                       const int* __restrict__ labels, const int* __restrict__ members,
                                                       const int* __restrict__ moffs, const double* __restrict__ cum_p,
                                                       int n_clusters, double lstar, unsigned gen,
                                                       int num_repeats, double* __restrict__ X_new, double* __restrict__ y_new,
                                                       int64_t* __restrict__ ncalls, int thin, int n_ph,
                                                       double* __restrict__ X_ph, double* __restrict__ y_ph) {
    __shared__ double r2s[MEAN_SLICE_CH];
    __shared__ double red[256];
    __shared__ double s_W[GPRY_MAX_DIM * GPRY_MAX_DIM];
    __shared__ double s_x[GPRY_MAX_DIM], s_u[GPRY_MAX_DIM], s_v[GPRY_MAX_DIM], s_z[GPRY_MAX_DIM];
    __shared__ double s_xt[GPRY_MAX_DIM], s_ut[GPRY_MAX_DIM];
    __shared__ double s_y;
    const int t = threadIdx.x, d = kp.d;
    const unsigned c = blockIdx.x;
    // the starting survivor
    const NsU2 us = ns_philox(a.seed, NS_PHASE_START, 0u, gen, c, 0u);
    int64_t j;
    const double* Wc = W;
    if (members) {
        const double u1 = ns_philox(a.seed, NS_PHASE_START, 1u, gen, c, 0u).a;
        int q = 0;
        while (q < n_clusters - 1 && !(u1 < cum_p[q])) q++;
        const int64_t nq = (int64_t)moffs[q + 1] - moffs[q];
        int64_t jq = (int64_t)(us.a * (double)nq);
        if (jq > nq - 1) jq = nq - 1;
        j = members[moffs[q] + jq];
        Wc = W + (int64_t)q * d * d;
    } else {
        j = (int64_t)(us.a * (double)nsurv);
        if (j > nsurv - 1) j = nsurv - 1;
        if (labels) Wc = W + (int64_t)labels[j] * d * d;
    }
    for (int e = t; e < d * d; e += 256) s_W[e] = Wc[e];
    double y_cur = y_surv[j];
    if (t < d) {
        s_x[t] = X_surv[j * d + t];
        s_u[t] = (s_x[t] - a.lo[t]) / (a.hi[t] - a.lo[t]);
    }
    __syncthreads();
    int64_t n_eval = 0;
    // the point at position tt along v: inside the box and above lstar?  (evaluates only inside the box)
    auto try_at = [&](double tt, double* y_out) -> bool {
        if (t < d) {
            const double u = s_u[t] + tt * s_v[t];
            s_ut[t] = u;
            s_xt[t] = a.lo[t] + u * (a.hi[t] - a.lo[t]);
        }
        __syncthreads();
        bool inside = true;
        for (int k = 0; k < d; k++)
            inside = inside && s_ut[k] >= 0.0 && s_ut[k] <= 1.0 && s_xt[k] >= a.lo[k] && s_xt[k] <= a.hi[k];
        if (!inside) { __syncthreads(); return false; }
        const double y = ns_eval<DP, KID>(s_xt, a, kp, ap, r2s, red, &s_y);
        n_eval++;
        *y_out = y;
        return y > lstar;
    };
    for (int s = 0; s < num_repeats; s++) {
        // direction
        if (t < (d + 1) / 2) ns_box_muller(s_z, t, d, ns_philox(a.seed, NS_PHASE_STEP, (unsigned)t, gen, c, (unsigned)s));
        __syncthreads();
        double nz = 0.0;
        for (int k = 0; k < d; k++) nz += s_z[k] * s_z[k];
        nz = sqrt(nz);
        if (t < d) {
            double v = 0.0;
            for (int k = 0; k <= t; k++) v += s_W[t * d + k] * s_z[k];
            s_v[t] = nz > 0.0 ? v / nz : 0.0;
        }
        __syncthreads();
        // stepping out
        const double r = ns_philox(a.seed, NS_PHASE_STEP, NS_DRAW_OFFSET, gen, c, (unsigned)s).a;
        double lt = -r, rt = 1.0 - r, yt = 0.0;
        for (int q = 0; q < NS_STEP_OUT_MAX && try_at(lt, &yt); q++) lt -= 1.0;
        for (int q = 0; q < NS_STEP_OUT_MAX && try_at(rt, &yt); q++) rt += 1.0;
        // shrinkage towards the current point (position 0)
        for (int q = 0; q < NS_SHRINK_MAX; q++) {
            const double u = ns_philox(a.seed, NS_PHASE_STEP, NS_DRAW_SHRINK + (unsigned)q, gen, c, (unsigned)s).a;
            const double tt = lt + u * (rt - lt);
            if (try_at(tt, &yt)) {
                if (t < d) { s_x[t] = s_xt[t]; s_u[t] = s_ut[t]; }
                y_cur = yt;
                break;
            }
            if (tt < 0.0) lt = tt; else rt = tt;
        }
        if (PH && (s + 1) % thin == 0 && s + 1 < num_repeats) {
            const int64_t r = (int64_t)c * n_ph + (s + 1) / thin - 1;
            if (t < d) X_ph[r * d + t] = s_x[t];
            if (t == 0) y_ph[r] = y_cur;
        }
        __syncthreads();
    }
    if (t < d) X_new[(int64_t)c * d + t] = s_x[t];
    if (t == 0) { y_new[c] = y_cur; ncalls[c] = n_eval; }
}

// ---- k nearest neighbours of the live set ----------------------------------------------------------------------------
struct NsBox { double lo[GPRY_MAX_DIM], hi[GPRY_MAX_DIM]; };

// u = (x - lo) / (hi - lo) as the chain kernel computes it, stored transposed (UT[k n + i]) so that neighbouring threads
// read neighbouring points
__global__ __launch_bounds__(256) void ns_unit_kernel(const double* __restrict__ X, NsBox b, int64_t n, int d,
                                                      double* __restrict__ UT) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * d) return;
    const int64_t i = e / d;
    const int k = (int)(e - i * d);
    UT[(int64_t)k * n + i] = (X[e] - b.lo[k]) / (b.hi[k] - b.lo[k]);
}

// squared distance of u_i (in LDS) and u_j: the squares rounded on their own (ns_rn) and added in coordinate order
__device__ __forceinline__ double ns_knn_d2(const double* __restrict__ UT, int64_t n, int d, const double* ui, int j) {
    double s = 0.0;
    for (int k = 0; k < d; k++) {
        const double df = ui[k] - UT[(int64_t)k * n + j];
        s = s + ns_rn(df * df);
    }
    return s;
}

// (da, ja) < (db, jb) lexicographically
__device__ __forceinline__ bool ns_knn_less(double da, int ja, double db, int jb) {
    return da < db || (da == db && ja < jb);
}

// Row i (one workgroup): its k nearest other points in order of (distance^2, index).  Round r selects the smallest key
// strictly above round r - 1's: a strided scan per thread, then a tree in LDS.  CACHE: the row's distances are computed
// once into LDS (n <= NS_KNN_LDS_N); otherwise every round recomputes them -- the same bits either way.
template <bool CACHE>
__global__ __launch_bounds__(256) void ns_knn_kernel(const double* __restrict__ UT, int n, int d, int k,
                                                     int* __restrict__ nbr) {
    extern __shared__ double s_dist[];
    __shared__ double s_ui[GPRY_MAX_DIM];
    __shared__ double r_d[256];
    __shared__ int r_j[256];
    const int t = threadIdx.x;
    const int i = blockIdx.x;
    if (t < d) s_ui[t] = UT[(int64_t)t * n + i];
    __syncthreads();
    if (CACHE) {
        for (int j = t; j < n; j += 256) s_dist[j] = ns_knn_d2(UT, n, d, s_ui, j);
        __syncthreads();
    }
    double last_d = -1.0;           // every distance is >= 0: the first round takes the smallest key
    int last_j = -1;
    for (int r = 0; r < k; r++) {
        double bd = INFINITY;
        int bj = INT_MAX;
        for (int j = t; j < n; j += 256) {
            if (j == i) continue;
            const double dj = CACHE ? s_dist[j] : ns_knn_d2(UT, n, d, s_ui, j);
            if (ns_knn_less(last_d, last_j, dj, j) && ns_knn_less(dj, j, bd, bj)) { bd = dj; bj = j; }
        }
        r_d[t] = bd;
        r_j[t] = bj;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w && ns_knn_less(r_d[t + w], r_j[t + w], r_d[t], r_j[t])) { r_d[t] = r_d[t + w]; r_j[t] = r_j[t + w]; }
            __syncthreads();
        }
        last_d = r_d[0];
        last_j = r_j[0];
        if (t == 0) nbr[(int64_t)i * k + r] = last_j;
        __syncthreads();
    }
}

// ---- one generation -------------------------------------------------------------------------------------------------
// What a generation is asked to do: the four gpry_ns_generation* entry points fill it in by name.
struct NsGenRequest {
    const char* who = nullptr;          // the entry point's name, for the messages
    bool need_labels = false, need_cum_p = false;      // the entry point requires them (the others take NULL for none)
    const double *lo = nullptr, *hi = nullptr, *X_surv = nullptr, *y_surv = nullptr, *W = nullptr;
    int64_t nsurv = 0, generation = 0; double lstar = 0.0; uint64_t seed = 0; int k = 0, num_repeats = 0;
    // clusters (labels NULL: none, one W); with cum_p the chains draw their cluster first
    const int32_t* labels = nullptr; int n_clusters = 1; const double* cum_p = nullptr;
    // phantoms (X_ph NULL: none)
    int thin = 1; double *X_ph = nullptr, *y_ph = nullptr;
    // outputs
    double *X_new = nullptr, *y_new = nullptr, *device_ms = nullptr; int64_t* ncalls = nullptr;
};

static int ns_check(gpry_ctx* ctx, const NsGenRequest& rq) {
    const char* who = rq.who;
    const int32_t* labels = rq.labels; const double* cum_p = rq.cum_p;
    const int64_t nsurv = rq.nsurv; const int n_clusters = rq.n_clusters;
    if (!ctx) return gpry_fail(nullptr, -1, "%s: ctx is NULL", who);
    if ((rq.need_labels && !labels) || (rq.need_cum_p && !cum_p)) return gpry_fail(ctx, -1, "%s: NULL argument", who);
    if (cum_p && nsurv > INT_MAX) return gpry_fail(ctx, -1, "%s: nsurv = %lld", who, (long long)nsurv);  // (int32 lists)
    if (!rq.lo || !rq.hi || !rq.X_surv || !rq.y_surv || !rq.W || !rq.X_new || !rq.y_new || !rq.ncalls)
        return gpry_fail(ctx, -1, "%s: NULL argument", who);
    if (rq.thin < 1) return gpry_fail(ctx, -1, "%s: thin = %d", who, rq.thin);
    if ((rq.X_ph == nullptr) != (rq.y_ph == nullptr))
        return gpry_fail(ctx, -1, "%s: X_ph and y_ph are both NULL or both given", who);
    if (nsurv < 1 || rq.k < 0 || rq.num_repeats < 0 || rq.generation < 0 || rq.generation > 0xffffffffll)
        return gpry_fail(ctx, -1, "%s: nsurv = %lld, k = %d, num_repeats = %d, generation = %lld", who,
                         (long long)nsurv, rq.k, rq.num_repeats, (long long)rq.generation);
    if (labels) {
        if (n_clusters < 1 || n_clusters > nsurv)
            return gpry_fail(ctx, -1, "%s: n_clusters = %d for %lld survivors", who, n_clusters, (long long)nsurv);
        for (int64_t i = 0; i < nsurv; i++)
            if (labels[i] < 0 || labels[i] >= n_clusters)
                return gpry_fail(ctx, -1, "%s: labels[%lld] = %d outside 0 .. %d", who, (long long)i, (int)labels[i],
                                 n_clusters - 1);
    }
    if (cum_p) {
        if (!labels) return gpry_fail(ctx, -1, "%s: cum_p without labels", who);
        for (int q = 0; q < n_clusters; q++)
            if (!(cum_p[q] >= (q ? cum_p[q - 1] : 0.0)))
                return gpry_fail(ctx, -1, "%s: cum_p[%d] = %.17g is not non-decreasing (nor >= 0)", who, q, cum_p[q]);
        if (cum_p[n_clusters - 1] != 1.0)
            return gpry_fail(ctx, -1, "%s: cum_p[%d] = %.17g, not 1.0", who, n_clusters - 1, cum_p[n_clusters - 1]);
        std::vector<int64_t> cnt(n_clusters, 0);
        for (int64_t i = 0; i < nsurv; i++) cnt[labels[i]]++;
        for (int q = 0; q < n_clusters; q++)
            if (cum_p[q] > (q ? cum_p[q - 1] : 0.0) && cnt[q] == 0)
                return gpry_fail(ctx, -1, "%s: cluster %d has probability %.17g and no survivor", who, q,
                                 cum_p[q] - (q ? cum_p[q - 1] : 0.0));
    }
    return 0;
}

// each cluster's survivors in their order in X_surv (a counting sort, stable by index): those of cluster q are
// mem[mof[q] .. mof[q + 1])
static void ns_members(const int32_t* labels, int64_t nsurv, int n_clusters, int32_t* mem, int32_t* mof) {
    for (int q = 0; q <= n_clusters; q++) mof[q] = 0;
    for (int64_t i = 0; i < nsurv; i++) mof[labels[i] + 1]++;
    for (int q = 0; q < n_clusters; q++) mof[q + 1] += mof[q];
    std::vector<int32_t> fill(mof, mof + n_clusters);
    for (int64_t i = 0; i < nsurv; i++) mem[fill[labels[i]]++] = (int32_t)i;
}

// a generation's arrays as the kernel sees them.  lab is used with labels alone; with cum_p the kernel reads the member
// lists mem / mof and cp instead; what is not used is NULL.  Xp / yp: the phantoms (NULL: not recorded).
struct NsGenDev {
    const double *Xs, *ys, *W; const int *lab, *mem, *mof; const double* cp;
    double *Xn, *yn; int64_t* cnt; double *Xp, *yp;
};

// the chain kernel of the context's (DP, KID), recording (PH) iff there is a phantom buffer
static void ns_launch_chains(gpry_ctx* ctx, const NsGenRequest& rq, const NsArgs& a, const KernParams& kp,
                             const AffParams& ap, const NsGenDev& g, int nw, int n_ph) {
#define NS_CHAIN(DP, KID, PH)                                                                                          \
    hipLaunchKernelGGL((ns_chain_kernel<DP, KID, PH>), dim3((unsigned)rq.k), dim3(256), 0, ctx->stream, a, kp, ap,      \
                       g.Xs, g.ys, rq.nsurv, g.W, g.lab, g.mem, g.mof, g.cp, nw, rq.lstar, (unsigned)rq.generation,    \
                       rq.num_repeats, g.Xn, g.yn, g.cnt, rq.thin, n_ph, g.Xp, g.yp)
#define NS_CHAIN_PLAIN(DP, KID) NS_CHAIN(DP, KID, false)
#define NS_CHAIN_PH(DP, KID) NS_CHAIN(DP, KID, true)
    if (g.Xp) { DISPATCH_DP_KID(ctx->d, ctx->kernel_id, NS_CHAIN_PH) }
    else { DISPATCH_DP_KID(ctx->d, ctx->kernel_id, NS_CHAIN_PLAIN) }
#undef NS_CHAIN_PH
#undef NS_CHAIN_PLAIN
#undef NS_CHAIN
}

static int ns_generation_impl(gpry_ctx* ctx, const NsGenRequest& rq) {
    GPRY_TRY(ns_check(ctx, rq));
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "nested sampler", rq.lo, rq.hi, rq.seed, &a, &kp, &ap));
    const int64_t d = ctx->d, n = rq.nsurv, k = rq.k, nc = rq.n_clusters, nw = rq.labels ? nc : 1;
    const bool lists = rq.cum_p != nullptr;
    // phantoms: n_ph recorded states per chain, [X_ph | y_ph] in the context's call scratch
    const int n_ph = rq.X_ph && rq.num_repeats > 0 ? (rq.num_repeats - 1) / rq.thin : 0;
    const int64_t psz[2] = {8 * k * n_ph * d, 8 * k * n_ph};
    if (psz[0] + psz[1] > NS_PHANTOM_MAX_BYTES)
        return gpry_fail(ctx, -1, "%s: %d chains x %d phantoms x %d coordinates need %lld bytes, the limit is %lld", rq.who,
                         rq.k, n_ph, (int)d, (long long)(psz[0] + psz[1]), (long long)NS_PHANTOM_MAX_BYTES);
    const bool rec = k > 0 && n_ph > 0;
    // ---- the pinned, mapped buffer: with cum_p the member lists and cum_p, else the labels if there are any
    std::vector<int32_t> mem, mof;
    if (lists) {
        mem.resize(n);
        mof.resize(nc + 1);
        ns_members(rq.labels, n, (int)nc, mem.data(), mof.data());
    }
    NsStage st(ctx, /*mapped=*/true);
    const auto rXs = st.in(rq.X_surv, n * d), rys = st.in(rq.y_surv, n), rW = st.in(rq.W, nw * d * d);
    const auto rcp = st.in(rq.cum_p, nc);
    const auto rlab = st.in(lists ? nullptr : rq.labels, n);
    const auto rmem = st.in(mem.data(), (int64_t)mem.size()), rmof = st.in(mof.data(), (int64_t)mof.size());
    const auto rXn = st.out(rq.X_new, k * d), ryn = st.out(rq.y_new, k);
    const auto rcnt = st.out(rq.ncalls, k);
    GPRY_TRY(st.begin());
    // ---- launch
    // the call scratch: the phantoms alone, claimed only where they are recorded (a generation without them holds nothing, and
    // both regions are empty).  Nothing else of this call claims it -- the stage lives in the pinned buffer -- and every
    // launch and copy is on ctx->stream, which st.end() drains.
    CallScratch cs(ctx, rq.who);
    const auto rXp = cs.take<double>(rec ? k * n_ph * d : 0), ryp = cs.take<double>(rec ? k * n_ph : 0);
    if (rec) GPRY_TRY(cs.claim());
    double *dXp = cs.at(rXp), *dyp = cs.at(ryp);
    const NsGenDev g = {st.dev(rXs), st.dev(rys), st.dev(rW), st.dev(rlab), st.dev(rmem), st.dev(rmof), st.dev(rcp),
                        st.dev(rXn), st.dev(ryn), st.dev(rcnt), dXp, dyp};
    if (k > 0) ns_launch_chains(ctx, rq, a, kp, ap, g, (int)nw, n_ph);
    // ---- copy back
    if (rec) {
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(rq.X_ph, dXp, (size_t)psz[0], hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(rq.y_ph, dyp, (size_t)psz[1], hipMemcpyDeviceToHost, ctx->stream));
    }
    return st.end(rq.device_ms);
}

// the part of a request that every generation entry point takes
static NsGenRequest ns_request(const char* who, const double* lo, const double* hi, const double* X_surv,
                               const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                               int64_t generation, int k, int num_repeats, double* X_new, double* y_new, int64_t* ncalls,
                               double* device_ms) {
    NsGenRequest rq;
    rq.who = who; rq.lo = lo; rq.hi = hi; rq.X_surv = X_surv; rq.y_surv = y_surv; rq.nsurv = nsurv; rq.lstar = lstar;
    rq.W = W; rq.seed = seed; rq.generation = generation; rq.k = k; rq.num_repeats = num_repeats;
    rq.X_new = X_new; rq.y_new = y_new; rq.ncalls = ncalls; rq.device_ms = device_ms;
    return rq;
}

extern "C" {

int gpry_ns_prior(gpry_ctx* ctx, const double* lo, const double* hi, uint64_t seed, int64_t n, double* X_out,
                  double* y_out, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_ns_prior: ctx is NULL");
    if (!lo || !hi || !X_out || !y_out) return gpry_fail(ctx, -1, "gpry_ns_prior: NULL argument");
    if (n < 0 || n > 0x7fffffffll) return gpry_fail(ctx, -1, "gpry_ns_prior: n = %lld", (long long)n);
    GPRY_TRY(require_model(ctx, true));
    NsArgs a; KernParams kp; AffParams ap;
    GPRY_TRY(ns_args(ctx, "nested sampler", lo, hi, seed, &a, &kp, &ap));
    NsStage st(ctx, /*mapped=*/true);
    const auto rX = st.out(X_out, n * ctx->d), ry = st.out(y_out, n);
    GPRY_TRY(st.begin());
#define NS_PRIOR(DP, KID)                                                                                          \
    hipLaunchKernelGGL((ns_prior_kernel<DP, KID>), dim3((unsigned)n), dim3(256), 0, ctx->stream, a, kp, ap, st.dev(rX), \
                       st.dev(ry))
    if (n > 0) { DISPATCH_DP_KID(ctx->d, ctx->kernel_id, NS_PRIOR) }
#undef NS_PRIOR
    return st.end(device_ms);
}

int gpry_ns_generation(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv, const double* y_surv,
                       int64_t nsurv, double lstar, const double* W, uint64_t seed, int64_t generation, int k,
                       int num_repeats, double* X_new, double* y_new, int64_t* ncalls, double* device_ms) {
    return ns_generation_impl(ctx, ns_request("gpry_ns_generation", lo, hi, X_surv, y_surv, nsurv, lstar, W, seed,
                                              generation, k, num_repeats, X_new, y_new, ncalls, device_ms));
}

int gpry_ns_generation_clustered(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                                 const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                                 int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                                 double* X_new, double* y_new, int64_t* ncalls, double* device_ms) {
    NsGenRequest rq = ns_request("gpry_ns_generation_clustered", lo, hi, X_surv, y_surv, nsurv, lstar, W, seed,
                                 generation, k, num_repeats, X_new, y_new, ncalls, device_ms);
    rq.labels = labels; rq.n_clusters = n_clusters; rq.need_labels = true;
    return ns_generation_impl(ctx, rq);
}

int gpry_ns_generation_volumes(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                               const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                               int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                               const double* cum_p, double* X_new, double* y_new, int64_t* ncalls, double* device_ms) {
    NsGenRequest rq = ns_request("gpry_ns_generation_volumes", lo, hi, X_surv, y_surv, nsurv, lstar, W, seed,
                                 generation, k, num_repeats, X_new, y_new, ncalls, device_ms);
    rq.labels = labels; rq.n_clusters = n_clusters; rq.cum_p = cum_p; rq.need_labels = rq.need_cum_p = true;
    return ns_generation_impl(ctx, rq);
}

int gpry_ns_generation_phantoms(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                                const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                                int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                                const double* cum_p, double* X_new, double* y_new, int64_t* ncalls, int thin, double* X_ph,
                                double* y_ph, double* device_ms) {
    NsGenRequest rq = ns_request("gpry_ns_generation_phantoms", lo, hi, X_surv, y_surv, nsurv, lstar, W, seed,
                                 generation, k, num_repeats, X_new, y_new, ncalls, device_ms);
    rq.labels = labels; rq.n_clusters = labels ? n_clusters : 1; rq.cum_p = cum_p;
    rq.thin = thin; rq.X_ph = X_ph; rq.y_ph = y_ph;
    return ns_generation_impl(ctx, rq);
}

int gpry_ns_knn(gpry_ctx* ctx, const double* lo, const double* hi, const double* X, int64_t n, int k, int32_t* nbr_out,
                double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_ns_knn: ctx is NULL");
    if (!lo || !hi || !X || !nbr_out) return gpry_fail(ctx, -1, "gpry_ns_knn: NULL argument");
    const int d = ctx->d;
    if (d < 1 || d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "gpry_ns_knn: d = %d outside 1 .. %d", d, GPRY_MAX_DIM);
    if (k < 1 || k > NS_KNN_MAX_K) return gpry_fail(ctx, -1, "gpry_ns_knn: k = %d outside 1 .. %d", k, NS_KNN_MAX_K);
    if (n < (int64_t)k + 1 || n > NS_KNN_MAX_N)
        return gpry_fail(ctx, -1, "gpry_ns_knn: n = %lld outside k + 1 = %d .. %d", (long long)n, k + 1, NS_KNN_MAX_N);
    NsBox b;
    for (int c = 0; c < GPRY_MAX_DIM; c++) {
        b.lo[c] = c < d ? lo[c] : 0.0;
        b.hi[c] = c < d ? hi[c] : 1.0;
        if (c < d && !(lo[c] < hi[c]) )
            return gpry_fail(ctx, -1, "gpry_ns_knn: bounds of dimension %d are [%g, %g]", c, lo[c], hi[c]);
    }
    // a non-finite coordinate would make the order undefined: refuse it rather than return a table
    for (int64_t e = 0; e < n * d; e++) {
        const int c = (int)(e % d);
        if (!isfinite((X[e] - b.lo[c]) / (b.hi[c] - b.lo[c])))
            return gpry_fail(ctx, -1, "gpry_ns_knn: point %lld has a non-finite unit-cube coordinate %d", (long long)(e / d), c);
    }
    // the call scratch: the transposed unit-cube points, the points as given, the neighbour table.  No other claimant is
    // called from here, and everything is queued on ctx->stream, which ns_end drains.
    CallScratch cs(ctx, "gpry_ns_knn");
    const auto rUT = cs.take<double>(n * d), rX = cs.take<double>(n * d); const auto rnbr = cs.take<int>(n * k);
    GPRY_TRY(cs.claim());
    double *dUT = cs.at(rUT), *dX = cs.at(rX);
    int* dnbr = cs.at(rnbr);
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    HIP_TRY(ctx, hipMemcpyAsync(dX, X, sizeof(double) * n * d, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ns_unit_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256), 0, ctx->stream, dX, b, n, d, dUT);
    if (n <= NS_KNN_LDS_N)
        hipLaunchKernelGGL(ns_knn_kernel<true>, dim3((unsigned)n), dim3(256), sizeof(double) * n, ctx->stream, dUT, (int)n,
                           d, k, dnbr);
    else
        hipLaunchKernelGGL(ns_knn_kernel<false>, dim3((unsigned)n), dim3(256), 0, ctx->stream, dUT, (int)n, d, k, dnbr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(nbr_out, dnbr, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost, ctx->stream));
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    return 0;
}

}  // extern "C"
