// What api.hip, sweep.hip and sweep_topk.hip share: the candidate sweep as the entry points see it.
#pragma once
#include "common.h"

// temporary device buffer of an entry point: freed on EVERY return path (the error paths of the entry points
// used to leak their scratch allocations)
template <typename T>
struct TmpBuf {
    T* p = nullptr;
    TmpBuf() = default;
    TmpBuf(const TmpBuf&) = delete;
    TmpBuf& operator=(const TmpBuf&) = delete;
    ~TmpBuf() { if (p) (void)hipFree(p); }
    int alloc(gpry_ctx* ctx, int64_t count) { return dev_alloc(ctx, &p, count); }
};

static inline int ensure_part(gpry_ctx* ctx, int64_t need) { return dev_grow(ctx, &ctx->dpart, &ctx->part_cap, need); }

// A pruned sweep (option "sweep_prune"): the sigma of a candidate that is not (yet) contracted.  No evaluated std takes this
// value (sqrt(var) * y_std >= 0, or NaN), so a shortlist record with it is known to carry a bound, not an exact acquisition.
#define PRUNED_SIGMA (-1.0)

// What run_sweep is asked to do with the candidates resident in ctx->dXc.
enum SweepKind {
    SWEEP_PREDICT,      // gpry_predict: y and (want_std) sigma, no acquisition; a batch of one chunk may take the split-K contraction
    SWEEP_FULL,         // the NORA sweep: y, sigma and the acquisition of every candidate
    SWEEP_STAGE_A       // stage A of a pruned sweep: the same panel-form decision and the same panel kernels, but the panel is
                        // not stored and nothing is contracted: y, the bound ub (ctx->dub) and the initial acq / sigma
};
struct SweepRequest {
    SweepKind kind = SWEEP_FULL;
    bool have_mask = false;
    bool want_std = true;       // (SWEEP_PREDICT only: the sweeps always compute sigma)
    // y is the caller's, resident in ctx->dy_all (or going up chunk by chunk from ctx->up_y): the panel is built without mean
    // partials and finished by sweep_given_finish_kernel; in stage A, sweep_given_bound_kernel alone (the panel-form decision
    // is still taken from the model: the contraction rounds build the panel in that form)
    bool y_given = false;
    double zeta = 0.0, baseline = 0.0, sigma_n = 0.0;
};
int run_sweep(gpry_ctx* ctx, int64_t M, const SweepRequest& rq);
int upload_candidates(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, bool upload_later = false);
// acq[i] = LogExp.f(mu[i], sd[i]) for n device values, on ctx->stream
int launch_logexp(gpry_ctx* ctx, const double* mu, const double* sd, int64_t n, double zeta, double baseline, double sigma_n, double* acq);
// pruned sweep: exact sigma / acq (and y after the bound pass) of the n candidates whose pool indices are in ctx->dgidx ...
int prune_eval(gpry_ctx* ctx, int64_t n);
int prune_complete(gpry_ctx* ctx);      // ... and of every candidate not contracted yet: the resident arrays become the full sweep's
