// What the device samplers of the surrogate's mean share: nested.hip (nested sampling), mcmc.hip (Metropolis),
// mcmc_ladders.hip (tempered Metropolis ladders) and hmc.hip (Hamiltonian Monte Carlo).  ns_eval is
// gpry_predict(x[None]) bit for bit (see nested.hip for the argument), ns_eval_multi the same for several points in one
// pass; ns_philox is the counter-based generator all draw from, restated in numpy by tests/tools/ns_philox.py.  Phases
// of the counter's word 0: 0-2 belong to the nested sampler (nested.hip), 3 to the Metropolis chains (mcmc.hip, and
// mcmc_ladders.hip, which adds draw 17 for its swaps), 4 to the Hamiltonian chains (hmc.hip), 5 to the joint draws of
// the surrogate (joint.hip: counter (5 << 24, draw s, pair j / 2, 0) gives z_s,2(j/2) and z_s,2(j/2)+1).
#pragma once
#include "kern_math.h"

#define NS_PHASE_JOINT 5u

struct NsU2 { double a, b; };

// the value of a product as it was rounded: an empty asm statement the combiner cannot look through, so that the sum
// it feeds is not fused into an FMA (-ffp-contract=fast) and rounds as the host's two operations do
__device__ __forceinline__ double ns_rn(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Philox4x32-10 (Salmon et al. 2011): two uniforms in [0, 1), 53 bits each, from words (0, 1) and (2, 3)
__device__ __forceinline__ NsU2 ns_philox(unsigned long long seed, unsigned phase, unsigned draw, unsigned gen,
                                          unsigned chain, unsigned step) {
    unsigned c0 = (phase << 24) | draw, c1 = gen, c2 = chain, c3 = step;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    NsU2 u;
    u.a = (double)((((unsigned long long)c0 << 32) | c1) >> 11) * 0x1.0p-53;
    u.b = (double)((((unsigned long long)c2 << 32) | c3) >> 11) * 0x1.0p-53;
    return u;
}

struct NsArgs {
    const double* Xs; const double* alpha_;
    int64_t rows_per_split;
    int nsplit, gates;
    double y_std, y_mean, clip_hi;
    GateParams gate;
    unsigned long long seed;
    double lo[GPRY_MAX_DIM], hi[GPRY_MAX_DIM];
};

// y of the point x (raw coordinates in LDS), valid in every thread.  Same slices, sums and finish as gpry_predict's
// one-point path (api.hip) and the resident kernel's (server.hip).
template <int DP, int KID>
__device__ double ns_eval(const double* x, const NsArgs& a, const KernParams& kp, const AffParams& ap, double* r2s,
                          double* red, double* s_y) {
    double mu = 0.0;
    for (int s = 0; s < a.nsplit; s++) {
        const double v = mean_slice<DP, KID>(x, a.Xs, a.alpha_, (int64_t)s * a.rows_per_split, a.rows_per_split, kp, ap, r2s, red);
        mu = mu + v;                         // (thread 0 holds the slice sums)
    }
    const unsigned bits = a.gates ? point_gate_bits(x, a.gate, kp, ap, red) : 0u;
    if (threadIdx.x == 0) {
        double y = fmin(ns_rn(mu * a.y_std) + a.y_mean, a.clip_hi);
        if (bits) y = -INFINITY;
        *s_y = y;
    }
    __syncthreads();
    const double y = *s_y;
    __syncthreads();
    return y;
}

// y of up to R points at once (point p: raw coordinates in LDS at x + p * GPRY_MAX_DIM; mask: bit p set = point p is
// evaluated, the same value in every thread): y[p] of every active point, valid in every thread, with the bits of
// ns_eval of that point alone -- mean_slice_multi's slices added from 0.0 in slice order, ns_eval's finish, the gates
// point by point.  A point that is masked out costs nothing and its y[p] is left as it was; with no active point there
// is no pass and no barrier.  r2s: R x MEAN_MULTI_CH doubles (also the gates' tree); s_y: R doubles.
template <int DP, int KID, int R>
__device__ __forceinline__ void ns_eval_multi(const double* x, unsigned mask, const NsArgs& a, const KernParams& kp,
                                              const AffParams& ap, double* r2s, double* s_y, double (&y)[R]) {
    if (!mask) return;
    double mu[R];
#pragma unroll
    for (int p = 0; p < R; p++) mu[p] = 0.0;
    for (int s = 0; s < a.nsplit; s++) {
        double v[R];
        mean_slice_multi<DP, KID, R>(x, mask, a.Xs, a.alpha_, (int64_t)s * a.rows_per_split, a.rows_per_split, kp, ap, r2s,
                                     v);
#pragma unroll
        for (int p = 0; p < R; p++)
            if (mask >> p & 1u) mu[p] = mu[p] + v[p];          // (thread 0 holds the slice sums)
    }
    unsigned gated = 0;
    if (a.gates) {
#pragma unroll
        for (int p = 0; p < R; p++)
            if ((mask >> p & 1u) && point_gate_bits(x + p * GPRY_MAX_DIM, a.gate, kp, ap, r2s)) gated |= 1u << p;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < R; p++) {
            if (!(mask >> p & 1u)) continue;
            double yy = fmin(ns_rn(mu[p] * a.y_std) + a.y_mean, a.clip_hi);
            if (gated >> p & 1u) yy = -INFINITY;
            s_y[p] = yy;
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < R; p++)
        if (mask >> p & 1u) y[p] = s_y[p];
    __syncthreads();
}

// What the two chain kernels (ns_chain_kernel, mcmc_chain_kernel) share beyond the above: the helper below and no more.
// The kernels differ on purpose in where products are fenced with ns_rn: the nested chain's W z sum and its
// lo + u * span may fuse into FMAs, the Metropolis chain's Lp z and lo + ns_rn(u * span) may not, and merging either
// pair changes bits.  The inside-the-box test over s_ut / s_xt is the same loop in both and stays written out in each:
// as a function of any form it compiles to other registers or other branches than the loop in place.
// Box-Muller: thread t < (d + 1) / 2 turns draw t of a step (u) into coordinates 2t and 2t + 1 of z ~ N(0, I) in LDS.  The
// draw stays with the caller (with it in here the chain kernel compiles to other code); the caller's barrier follows.
__device__ __forceinline__ void ns_box_muller(double* s_z, int t, int d, NsU2 u) {
    const double rad = sqrt(-2.0 * log(1.0 - u.a)), ang = 6.283185307179586 * u.b;
    s_z[2 * t] = rad * cos(ang);
    if (2 * t + 1 < d) s_z[2 * t + 1] = rad * sin(ang);
}

// ---- host side -----------------------------------------------------------------------------------
// byte offsets of N regions of sz[i] bytes laid end to end, each on a 256-byte boundary: off[i], and off[N] for the whole
template <int N>
static void ns_layout(const int64_t (&sz)[N], int64_t (&off)[N + 1]) {
    off[0] = 0;
    for (int i = 0; i < N; i++) off[i + 1] = off[i] + round_up(sz[i], 256);
}

static int ns_args(gpry_ctx* ctx, const char* who, const double* lo, const double* hi, unsigned long long seed, NsArgs* a, KernParams* kp,
                   AffParams* ap) {
    if (ctx->d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "%s: d = %d > %d", who, ctx->d, GPRY_MAX_DIM);
    GPRY_TRY(ensure_pred_xs(ctx));
    *kp = make_kp(ctx);
    *ap = make_ap(ctx, kp->has_aff);
    int nsplit = (int)(ctx->N / 1024);            // the slices of the one-point path (api.hip: gpry_predict)
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 8) nsplit = 8;
    a->Xs = ctx->dXs; a->alpha_ = ctx->dalpha_;
    a->nsplit = nsplit;
    a->rows_per_split = round_up((ctx->N + nsplit - 1) / nsplit, 32);
    a->gates = ctx->gates_on;
    a->gate = make_gp(ctx);
    a->y_std = ctx->tf.y_std; a->y_mean = ctx->tf.y_mean; a->clip_hi = ctx->tf.clip_hi;
    a->seed = seed;
    for (int k = 0; k < GPRY_MAX_DIM; k++) {
        a->lo[k] = k < ctx->d ? lo[k] : 0.0;
        a->hi[k] = k < ctx->d ? hi[k] : 1.0;
        if (k < ctx->d && !(lo[k] < hi[k]))
            return gpry_fail(ctx, -1, "%s: bounds of dimension %d are [%g, %g]", who, k, lo[k], hi[k]);
    }
    return 0;
}

struct NsTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~NsTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

static int ns_begin(gpry_ctx* ctx, NsTimer* tm) {
    GPRY_TRY(serve_stop(ctx));          // the resident predict kernel would share the CUs
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventCreate(&tm->e0));
    HIP_TRY(ctx, hipEventCreate(&tm->e1));
    HIP_TRY(ctx, hipEventRecord(tm->e0, ctx->stream));
    return 0;
}

static int ns_end(gpry_ctx* ctx, NsTimer* tm, double* device_ms) {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(tm->e1, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, tm->e0, tm->e1));
    if (device_ms) *device_ms = ms;
    return 0;
}

// The staged buffer of one call: an entry point declares its inputs (in) and outputs (out) in any order, begin() lays
// them end to end on 256-byte boundaries and uploads the inputs, dev() gives the kernel its pointers, end() brings every
// output back to its host array and times the call.  A region whose host pointer is NULL or whose count is 0 has no
// bytes, dev() == nullptr and no copy.  An output may start filled with a byte (0xff: NaN and -1).
// Backing, chosen at construction: the context's device buffer (dmc), with asynchronous copies between the two events, or
// (mapped) its pinned, mapped buffer (hpin), with memcpy in before the first event and out after the synchronise.
struct NsStage {
    template <class T> struct In { int i; };
    template <class T> struct Out { int i; };
    struct Region { const void* src; void* dst; int64_t bytes, off; int fill; };
    static const int CAP = 24;
    gpry_ctx* ctx; bool mapped;
    Region r[CAP + 1];                  // (slot CAP: where a region beyond the capacity lands; begin() then fails)
    int n = 0;
    int64_t total = 0;
    char* base = nullptr;               // the buffer as the device sees it
    NsTimer tm;

    NsStage(gpry_ctx* c, bool m = false) : ctx(c), mapped(m) {}
    int add(const void* src, void* dst, bool given, int64_t bytes, int fill) {
        const int i = n < CAP ? n : CAP;
        r[i] = {src, dst, given ? bytes : 0, total, fill};
        total += round_up(r[i].bytes, 256);
        n++;
        return i;
    }
    template <class T> In<T> in(const T* p, int64_t count) { return {add(p, nullptr, p != nullptr, (int64_t)sizeof(T) * count, -1)}; }
    template <class T> Out<T> out(T* p, int64_t count, int fill = -1) {
        return {add(nullptr, p, p != nullptr, (int64_t)sizeof(T) * count, fill)};
    }
    template <class T> const T* dev(In<T> h) const { return r[h.i].bytes ? (const T*)(base + r[h.i].off) : nullptr; }
    template <class T> T* dev(Out<T> h) const { return r[h.i].bytes ? (T*)(base + r[h.i].off) : nullptr; }

    // the buffer, the inputs and the fills, and the first event
    int begin() {
        if (n > CAP) return gpry_fail(ctx, -1, "NsStage: %d regions, the table holds %d", n, CAP);
        if (mapped) {
            GPRY_TRY(ensure_pinned(ctx, total));
            base = (char*)ctx->hpin_dev;
            char* h = (char*)ctx->hpin;
            for (int i = 0; i < n; i++) {
                if (r[i].bytes && r[i].src) memcpy(h + r[i].off, r[i].src, r[i].bytes);
                if (r[i].bytes && r[i].fill >= 0) memset(h + r[i].off, r[i].fill, r[i].bytes);
            }
            return ns_begin(ctx, &tm);
        }
        GPRY_TRY(ns_begin(ctx, &tm));
        GPRY_TRY(dev_grow(ctx, &ctx->dmc, &ctx->mc_cap, total));
        base = (char*)ctx->dmc;
        for (int i = 0; i < n; i++) {
            if (r[i].bytes && r[i].src)
                HIP_TRY(ctx, hipMemcpyAsync(base + r[i].off, r[i].src, r[i].bytes, hipMemcpyHostToDevice, ctx->stream));
            if (r[i].bytes && r[i].fill >= 0) HIP_TRY(ctx, hipMemsetAsync(base + r[i].off, r[i].fill, r[i].bytes, ctx->stream));
        }
        return 0;
    }
    // the launch's error, the outputs, the second event, the synchronise and device_ms
    int end(double* device_ms) {
        if (!mapped) {
            HIP_TRY(ctx, hipGetLastError());
            for (int i = 0; i < n; i++)
                if (r[i].bytes && r[i].dst)
                    HIP_TRY(ctx, hipMemcpyAsync(r[i].dst, base + r[i].off, r[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        GPRY_TRY(ns_end(ctx, &tm, device_ms));
        if (mapped)
            for (int i = 0; i < n; i++)
                if (r[i].bytes && r[i].dst) memcpy(r[i].dst, (const char*)ctx->hpin + r[i].off, r[i].bytes);
        return 0;
    }
};

// ---- the checks the point-batch entry points share (hessian.hip, joint.hip, theta_grad.hip, predict_thetas.hip,
// predict_without.hip, var_theta_grad.hip): every coordinate of the npts rows of X is finite ...
static int check_points_finite(gpry_ctx* ctx, const char* who, const double* X, int64_t npts) {
    const int d = ctx->d;
    for (int64_t e = 0; e < npts * d; e++)
        if (!isfinite(X[e])) return gpry_fail(ctx, -1, "%s: a coordinate of point %lld is not finite", who, (long long)(e / d));
    return 0;
}
// ... and the x-affine map, where the model has one, divides by a finite non-zero span
static int check_x_affine(gpry_ctx* ctx, const char* who) {
    if (!ctx->tf.has_x_affine) return 0;
    for (int k = 0; k < ctx->d; k++)
        if (!(ctx->tf.x_span[k] != 0.0) || !isfinite(ctx->tf.x_span[k]) || !isfinite(ctx->tf.x_lo[k]))
            return gpry_fail(ctx, -1, "%s: affine map of X: span %g, offset %g in dimension %d", who, ctx->tf.x_span[k],
                             ctx->tf.x_lo[k], k);
    return 0;
}

// ---- the argument checks the chain entry points share (mcmc.hip, mcmc_ladders.hip, hmc.hip) --------
// rung < 0: the one temperature of a plain chain call
static int ns_check_temperature(gpry_ctx* ctx, const char* who, double T, int rung = -1) {
    if (T > 0.0 && isfinite(T)) return 0;
    if (rung < 0) return gpry_fail(ctx, -1, "%s: temperature T = %g", who, T);
    return gpry_fail(ctx, -1, "%s: temperature T[%d] = %g", who, rung, T);
}

// nrungs = 0: nchains plain chains at the temperature T[0]; nrungs >= 1 (already in range): nchains ladders of nrungs
// chains at the temperatures T[0 .. nrungs)
static int ns_check_chains(gpry_ctx* ctx, const char* who, int64_t nchains, int nrungs, int nsteps, int thin, int64_t batch,
                           const double* T, const void* X_rec, const void* y_rec, const void* X_prop, const void* y_prop) {
    if ((X_prop == nullptr) != (y_prop == nullptr))
        return gpry_fail(ctx, -1, "%s: X_prop and y_prop are both NULL or both given", who);
    if (nchains < 1 || nchains * (nrungs ? nrungs : 1) > 0x7fffffffll || nsteps < 0 || thin < 1 || batch < 0 ||
        batch > 0xffffffffll) {
        if (nrungs)
            return gpry_fail(ctx, -1, "%s: nladders = %lld, nrungs = %d, nsteps = %d, thin = %d, batch = %lld", who,
                             (long long)nchains, nrungs, nsteps, thin, (long long)batch);
        return gpry_fail(ctx, -1, "%s: nchains = %lld, nsteps = %d, thin = %d, batch = %lld", who, (long long)nchains, nsteps,
                         thin, (long long)batch);
    }
    if (!nrungs) GPRY_TRY(ns_check_temperature(ctx, who, T[0]));
    for (int r = 0; r < nrungs; r++) GPRY_TRY(ns_check_temperature(ctx, who, T[r], r));
    if (nsteps / thin > 0 && (!X_rec || !y_rec)) return gpry_fail(ctx, -1, "%s: NULL argument", who);
    return 0;
}

