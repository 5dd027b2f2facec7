// C-ABI entry points of the GP hot path (include/gpry_hip.h): factor, LML, predict, gates and Kriging-believer support
// (the NORA sweep: sweep.hip; its shortlist selection: sweep_topk.hip).
#include "sweep.h"
#include "kb_gram.h"
#include <algorithm>

int require_model(gpry_ctx* ctx, bool need_factor) {
    if (ctx->N <= 0) return gpry_fail(ctx, -1, "no training set (call gpry_set_train)");
    if (!ctx->have_theta) return gpry_fail(ctx, -1, "no hyperparameters (call gpry_set_theta)");
    if (need_factor && !ctx->factor_valid) return gpry_fail(ctx, -1, "model not factorised (call gpry_factorize)");
    // an X map that was set for a model of fewer dimensions has zero spans in the new ones: every prediction would be NaN
    if (need_factor && ctx->tf.has_x_affine)
        for (int k = 0; k < ctx->d; k++)
            if (!(ctx->tf.x_span[k] != 0.0) || !isfinite(ctx->tf.x_span[k]) || !isfinite(ctx->tf.x_lo[k]))
                return gpry_fail(ctx, -1, "affine map of X: span %g, offset %g in dimension %d of %d (gpry_set_affine of another model?)",
                                 ctx->tf.x_span[k], ctx->tf.x_lo[k], k, ctx->d);
    return 0;
}


// copy a device matrix with leading dimension ld to a dense host rows x cols array
static int copy_out_matrix(gpry_ctx* ctx, const double* dsrc, int64_t ld, int64_t rows, int64_t cols, double* hdst) {
    HIP_TRY(ctx, hipMemcpy2DAsync(hdst, sizeof(double) * cols, dsrc, sizeof(double) * ld,
                                  sizeof(double) * cols, rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// A panel step whose bounded waits ran out (chol_panel.hip: PANEL_SPIN_CAP) reports a failing column like a matrix that is
// not positive definite and leaves a marker in the fourth status word.  That is a scheduling failure, not a property of the
// matrix: the caller gets an error, never the -inf of sklearn's non-PD convention (an optimiser would go on with a wrong objective).
bool panel_timed_out(int marker) { return (marker & 0xFF00) == 0x5A00; }
int panel_timeout_error(gpry_ctx* ctx, int marker) {
    return gpry_fail(ctx, -2, "Cholesky panel step timed out (wait %d; the GPU is shared with work that starves the step?)", marker & 0xFF);
}

// ---- the protocol of an objective evaluation at thetas that are not the context's own (common.h) ------------------------
int objective_entry(gpry_ctx* ctx, const char* name, const double* thetas, int64_t B) {
    GPRY_TRY(serve_stop(ctx));
    if (ctx->N <= 0) return gpry_fail(ctx, -1, "%s: no training set (call gpry_set_train)", name);
    const int w = ctx_ntheta(ctx);      // 1 + d, one more (log w) for a model set with GPRY_KERNEL_WHITE
    for (int64_t i = 0; i < B * w; i++)
        if (!isfinite(thetas[i]))
            return gpry_fail(ctx, -1, "%s: theta[%d] of evaluation %lld is not finite", name, (int)(i % w), (long long)(i / w));
    if (ctx->d > 32) return gpry_fail(ctx, -1, "%s: d > 32 is not supported", name);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->lml_cache = false;
    return 0;
}
int objective_row(gpry_ctx* ctx, int64_t bytes, int info_at, double** hres, double** dres) {
    GPRY_TRY(ensure_pinned(ctx, bytes));
    *hres = static_cast<double*>(ctx->hpin);
    *dres = static_cast<double*>(ctx->hpin_dev);        // the same buffer as the device sees it
    objective_row_unwritten(*hres, info_at);
    return 0;
}
int objective_status(gpry_ctx* ctx, const char* name, int64_t which, const double* row, int info_at, int* info) {
    if (row[info_at] < 0.0) return gpry_fail(ctx, -2, "%s: evaluation %lld did not deliver its status", name, (long long)which);
    if (panel_timed_out((int)row[info_at + 2])) return panel_timeout_error(ctx, (int)row[info_at + 2]);
    const int i0 = (int)row[info_at], i1 = (int)row[info_at + 1];
    *info = i0 != 0 ? i0 : i1;
    return 0;
}
// The factorisation status is not waited for in the middle of a chain (every kernel behind a failed factorisation either
// exits on *dinfo != 0 or works on values nobody reads); status and results come back together at the end, written into the
// mapped row by the last kernels themselves (no copy-out operations behind the evaluation).
// (Polling the status word in the mapped buffer instead of waiting for the stream returns 15 us earlier and is WRONG: inbound
// PCIe writes to different cache lines are not ordered here -- the host saw the status before the last gradient entries in
// 2 % of the evaluations, tests/tools/stress_concurrent_fit.py; a loop over hipStreamQuery is correct and no faster than
// hipStreamSynchronize.)
int objective_wait(gpry_ctx* ctx, const char* name, int rc, const double* row, int info_at, int* info) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) return gpry_fail(ctx, -2, "%s: %s", name, hipGetErrorString(e));
    return row ? objective_status(ctx, name, 0, row, info_at, info) : 0;
}
void objective_write(const gpry_ctx* ctx, int info, double head, const double* g, const double* h, double* value, double* grad,
                     double* hess) {
    const int w = ctx_ntheta(ctx);
    const bool pd = info == 0;          // otherwise sklearn:_gpr.py:586-589
    *value = pd ? head - 0.5 * (double)ctx->N * log(2.0 * M_PI) : -INFINITY;
    if (grad) for (int k = 0; k < w; k++) grad[k] = pd ? g[k] : 0.0;
    if (hess) for (int k = 0; k < w * w; k++) hess[k] = pd ? h[k] : 0.0;
}

int build_factor(gpry_ctx* ctx, double* A, double* V, double* T, int* info_host) {
    // A <- K + diag(alpha); A <- chol(A) (lower); V <- A^-1
    GPRY_TRY(launch_scale_train(ctx));      // X / l (N x d, microseconds)
    // (where V comes out of the Cholesky launches -- potrf_stacked below -- T starts as the identity: written by the same kernel)
    const bool want_stacked = ctx->opt_chol != 1 && potrf_stacked_usable(ctx, ctx->Np);
    {
        StageScope s(ctx, "kernel_build");   // the O(N^2 d) covariance build proper
        GPRY_TRY(launch_kernel_train(ctx, A, 1, want_stacked ? T : nullptr));
    }
    if (ctx->opt_chol == 1) {
        StageScope s(ctx, "potrf");
        GPRY_TRY(rocsolver_potrf_trtri(ctx, A, V, ctx->Np, 1));
    } else {
        // V = L^-1 phase by phase on stream2 while the panel chain is still running (chol.hip); "trtri" then
        // times what is left of it after potrf
        bool piped = false;
        struct PipeGuard {      // an error between begin and finish must not leave side-stream work in flight
            gpry_ctx* c; bool armed = false;
            ~PipeGuard() { if (armed) trtri_pipeline_abort(c); }
        } guard{ctx};
        // (a batched evaluation has thetas enough to fill the GPU: its V = L^-1 stays behind potrf on the main stream;
        // the two schedules give the same bits)
        if (ctx->opt_factor_pipeline && ctx->opt_chol == 0 && ctx->Np >= ctx->opt_factor_pipeline_min && ctx->bn == 1 && !ctx->tp &&
            !potrf_stacked_usable(ctx, ctx->Np)) {
            const int rc = trtri_pipeline_begin(ctx, A, V, T, ctx->Np);
            if (rc < 0) return rc;
            piped = rc == 0;
            guard.armed = piped;
        }
        // Up to Np = "chol_stacked" the inverse factor comes out of the Cholesky launches themselves (potrf_stacked, chol_panel.hip):
        // T takes the identity and comes back as L^-T, which is transposed into V.
        bool stacked = !piped && want_stacked;
        if (stacked) {
            StageScope s(ctx, "potrf");
            const int rc = potrf_stacked(ctx, A, T, ctx->Np);
            if (rc < 0) return rc;
            stacked = rc == 0;      // (1: no plan for this size)
        }
        if (stacked) {
            StageScope s(ctx, "trtri");
            GPRY_TRY(transpose_upper_launch(ctx, T, V, ctx->Np));
        } else {
            {
                StageScope s(ctx, "potrf");
                GPRY_TRY(ctx->opt_chol_overlap ? potrf_lower_overlap(ctx, A, ctx->Np) : potrf_lower_fused(ctx, A, ctx->Np));
            }
            {
                StageScope s(ctx, "trtri");
                if (piped) { GPRY_TRY(trtri_pipeline_finish(ctx)); guard.armed = false; }
                else GPRY_TRY(trtri_lower(ctx, A, V, T, ctx->Np));
            }
        }
    }
    ctx->info_cleared = false;
    if (!info_host) return 0;      // the caller fetches dinfo itself, together with its results
    int info[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(info, ctx->dinfo, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (panel_timed_out(info[3])) return panel_timeout_error(ctx, info[3]);
    *info_host = info[0] != 0 ? info[0] : info[1];
    return 0;
}

// The launches of one objective evaluation (sklearn:_gpr.py:574-652) at the theta the context holds -- or, in a batched
// evaluation (gpry_ctx::bn), at the bn thetas whose [C, l...] rows sit in the arena: covariance build, factor, V = L^-1,
// alpha, log-det and quadratic form, and with want_grad K^-1 = V^T V and the traces.  The last kernel writes results and
// factorisation status into `dres` (device view of pinned host memory; theta tb at row tb of GPRY_BRES_STRIDE doubles).
constexpr int RES_INFO = LML_RES_INFO;            // [logdet/2, quad, grad (1 + d, + 1 with a white term) ..., info0, info1]
static_assert(RES_INFO + 3 <= GPRY_BRES_STRIDE, "result row too short");
int lml_chain(gpry_ctx* ctx, int want_grad, double* dres) {
    GPRY_TRY(build_factor(ctx, ctx->dW, ctx->dW2, ctx->dW3, nullptr));
    double* dz = ctx->dvec;                 // z = V y
    double* da = ctx->dvec + ctx->Np;       // alpha
    double* dout = ctx->dvec + 2 * ctx->Np; // device copy: [logdet/2, quad, grad...]
    {
        StageScope s(ctx, "solve_alpha");
        GPRY_TRY(solve_alpha(ctx, ctx->dW2, ctx->dy, dz, da, ctx->Np));
        GPRY_TRY(logdet_and_quad(ctx, ctx->dW, dz, ctx->Np, dout, want_grad ? nullptr : dres, RES_INFO));
    }
    if (!want_grad) return 0;
    {
        StageScope s(ctx, "lauum");
        GPRY_TRY(lauum_lower(ctx, ctx->dW2, ctx->dW3, ctx->Np));
    }
    StageScope s(ctx, "lml_traces");
    return launch_lml_traces(ctx, ctx->dW3, da, dout + 2, dout, dres, RES_INFO);
}

// ---- B thetas in ONE chain of launches (128 < Np <= lml_batch; the leave-one-out objective: from Np = 128) ----------
// The reference runs the optimiser restarts of a fit one after another (gpry/gpr.py:968-984, 10 + 2 d of them by default,
// gpry/run.py:315-325); stepped side by side (gpry_amd/lockstep.py) they hand a round's thetas to gpry_lml_batch.  Above
// N = 128 one evaluation is a chain of 20-60 launches that keeps a handful of CUs busy (0.001-0.02 of the FP64 peak at
// N = 256 ... 1024); here every launch of that chain carries all thetas (grid.z).  Same kernels, same launch geometry,
// same operands per theta as a single gpry_lml: the per-theta results are bit-identical to it.
struct BatchLayout {
    int64_t w, w2, w3, xs, vec, part, split, par, info;     // offsets (doubles) within a theta's set
    int64_t part_cap, split_cap, stride;
};
// (bc.part_min / bc.split_min: what the chain's own tail needs of the two shared pieces; 0 for the LML, whose layout is the
// factor chain's)
static int batch_layout(gpry_ctx* ctx, const BatchChain& bc, BatchLayout* L) {
    const int64_t Np = ctx->Np, nn = Np * Np;
    int slices = 0;
    GPRY_TRY(factor_chain_slices(ctx, Np, &slices));
    const int DPsel = dp_class(ctx->d);
    const int64_t nb = Np / 64, ntile = nb * (nb + 1) / 2;
    const int64_t p1 = ((Np + 255) / 256) * Np, p2 = ntile * (DPsel + 2);       // solve_alpha, launch_lml_traces
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o += round_up(n, 32); return at; };      // 256-byte pieces
    L->w = take(nn); L->w2 = take(nn); L->w3 = take(nn);
    L->xs = take(Np * ctx->dpad);
    L->vec = take(8 * Np + 4096);
    L->part_cap = p1 > p2 ? p1 : p2;
    if (L->part_cap < bc.part_min) L->part_cap = bc.part_min;
    L->part = take(L->part_cap);
    L->split_cap = (int64_t)slices * nn;
    if (L->split_cap < bc.split_min) L->split_cap = bc.split_min;
    L->split = take(L->split_cap > 0 ? L->split_cap : 1);
    L->par = take(GPRY_BPAR_ROW);
    L->info = take(8);                      // 16 status / arrival words
    L->stride = o + 32 * 9;                 // not a multiple of a large power of two: consecutive sets start on different channels
    return 0;
}
// returns 2 when the device has no room for the arena (the caller halves its chunk), < 0 on any other failure
static int ensure_batch_buffers(gpry_ctx* ctx, int64_t arena_doubles, int64_t res_bytes) {
    if (arena_doubles > ctx->barena_cap) {
        if (ctx->barena) GPRY_TRY(dev_free(ctx, ctx->barena));
        ctx->barena = nullptr; ctx->barena_cap = 0;
        const hipError_t e = hipMalloc((void**)&ctx->barena, sizeof(double) * (size_t)arena_doubles);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); ctx->barena = nullptr; return 2; }
        if (e != hipSuccess) { ctx->barena = nullptr; return gpry_fail(ctx, -2, "batched objective: hipMalloc of the scratch arena failed: %s", hipGetErrorString(e)); }
        ctx->barena_cap = arena_doubles;
    }
    if (res_bytes > ctx->hbres_cap) {
        if (ctx->hbres) HIP_TRY(ctx, hipHostFree(ctx->hbres));
        ctx->hbres = nullptr; ctx->hbres_dev = nullptr; ctx->hbres_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->hbres, (size_t)res_bytes, hipHostMallocMapped | hipHostMallocPortable));
        HIP_TRY(ctx, hipHostGetDevicePointer(&ctx->hbres_dev, ctx->hbres, 0));
        memset(ctx->hbres, 0, (size_t)res_bytes);
        ctx->hbres_cap = res_bytes;
    }
    return 0;
}
// is the batched chain built for this context's size and options?  (rocSOLVER is not batched: one evaluation after another)
static bool lml_batch_usable(const gpry_ctx* ctx) {
    return ctx->N > 0 && ctx->Np > 128 && ctx->Np <= ctx->opt_lml_batch && ctx->d <= 32 && ctx->opt_chol == 0;
}
// the LML's chain as objective_batch_general runs it (gpry_loo_objective_batch hands in its own: loo_fit.hip)
static const BatchChain LML_BATCH = {"lml_batch", lml_chain, false, 0, 0, 2, RES_INFO, lml_head};
int objective_batch_general(gpry_ctx* ctx, const BatchChain& bc, const double* thetas, int64_t B, int want_grad, double* lml, double* grad,
                            int* info) {
    const int w = ctx_ntheta(ctx);      // (the caller has run objective_entry on the thetas)
    // the chain below is the code of a single evaluation: it finds the buffers of theta 0 where the context keeps its own
    struct Scope {
        gpry_ctx* c;
        double *dW, *dW2, *dW3, *dXs, *dvec, *dpart, *dsplit; int* dinfo; hipStream_t stream;
        int64_t part_cap, split_cap; bool xs_foreign, have_theta;
        double theta[GPRY_THETA_MAX];
        explicit Scope(gpry_ctx* ctx) : c(ctx), dW(ctx->dW), dW2(ctx->dW2), dW3(ctx->dW3), dXs(ctx->dXs), dvec(ctx->dvec), dpart(ctx->dpart),
                                        dsplit(ctx->dsplit), dinfo(ctx->dinfo), stream(ctx->stream), part_cap(ctx->part_cap), split_cap(ctx->split_cap),
                                        xs_foreign(ctx->xs_foreign), have_theta(ctx->have_theta) {
            memcpy(theta, ctx->theta, sizeof(theta));
        }
        ~Scope() {
            c->dW = dW; c->dW2 = dW2; c->dW3 = dW3; c->dXs = dXs; c->dvec = dvec; c->dpart = dpart; c->dsplit = dsplit; c->dinfo = dinfo;
            c->stream = stream;
            c->part_cap = part_cap; c->split_cap = split_cap; c->xs_foreign = xs_foreign; c->have_theta = have_theta;
            c->info_cleared = false;
            memcpy(c->theta, theta, sizeof(theta));
            c->bn = 1; c->bstride = 0; c->bpar = nullptr; c->tp = false;
        }
    } scope(ctx);
    // THE THROUGHPUT SCHEDULE (option "lml_schedule" = 1; gpry_ctx::opt_lml_schedule): whole-tile products only, the recursive
    // inverse at every size, the Cholesky in column blocks, the thetas of a chunk dealt over stream groups.  Everything a theta's
    // result depends on is a function of the model size alone -- never of B, of the chunking or of the grouping.
    // (a chain without that form -- the leave-one-out objective's -- runs the latency schedule whatever the option says)
    const bool tp = !bc.latency_only && ctx->opt_lml_schedule == 1;
    ctx->tp = tp;
    BatchLayout L;
    GPRY_TRY(batch_layout(ctx, bc, &L));
    // thetas per chain: the diagonal workgroup of a panel step waits for the other workgroups of ITS theta to have read the
    // block it overwrites -- only those wait, one per theta, so any number well below the GPU's workgroup slots is safe
    int64_t chunk = B < 96 ? B : 96;
    int64_t mem_cap = (ctx->opt_lml_batch_mb << 20) / (8 * L.stride);
    {
        // ... and by what the device has free right now: a fit opens up to three such contexts per GPU beside the farm's,
        // and "lml_batch_mb" is sized for an empty 288-GB part.  The arena may take what it already holds plus 70 % of
        // the free memory.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const int64_t room = ctx->barena_cap * 8 + (int64_t)((double)free_b * 0.7);
            if (room / (8 * L.stride) < mem_cap) mem_cap = room / (8 * L.stride);
        }
    }
    if (chunk > mem_cap) chunk = mem_cap;
    // (latency schedule: below two sets the caller evaluates the thetas one after another -- the same bits; the throughput
    // schedule has no such twin: one set at a time is still its own chain)
    const int64_t min_chunk = tp ? 1 : 2;
    if (chunk < min_chunk) {
        if (!tp) return 1;
        return gpry_fail(ctx, -2, "%s: no device memory for one scratch set (%lld MiB)", bc.name, (long long)((8 * L.stride) >> 20));
    }
    // a failed allocation (another context took the memory in between) halves the chunk; below `min_chunk` sets the thetas go
    // through one after another instead of the fit failing (latency schedule).  Only an out-of-memory answer is retried.
    for (;;) {
        const int rc = ensure_batch_buffers(ctx, chunk * L.stride, (int64_t)sizeof(double) * chunk * (GPRY_BRES_STRIDE + GPRY_BPAR_ROW));
        if (rc == 0) break;
        if (rc != 2) return rc;             // anything but "out of memory" is the caller's to see
        ctx->batch_shrinks++;
        chunk /= 2;
        if (chunk < min_chunk) {
            if (!tp) return 1;
            return gpry_fail(ctx, -2, "%s: no device memory for one scratch set", bc.name);
        }
    }
    ctx->batch_set_doubles = L.stride; ctx->batch_chunk = chunk;
    double* hres = static_cast<double*>(ctx->hbres);
    double* hpar = hres + chunk * GPRY_BRES_STRIDE;         // [C, l_1 .. l_d] rows of a chunk, staged in the pinned buffer
    double* a0 = ctx->barena;
    const hipStream_t main_stream = scope.stream;
    // the sets of thetas [t0, t0 + n) become "the context's own buffers" for the launchers of the chain
    auto point_at = [&](int64_t t0, int64_t n, hipStream_t st) {
        double* a = a0 + t0 * L.stride;
        ctx->dW = a + L.w; ctx->dW2 = a + L.w2; ctx->dW3 = a + L.w3; ctx->dXs = a + L.xs; ctx->dvec = a + L.vec;
        ctx->dpart = a + L.part; ctx->part_cap = L.part_cap; ctx->dsplit = a + L.split; ctx->split_cap = L.split_cap;
        ctx->dinfo = reinterpret_cast<int*>(a + L.info);
        ctx->bstride = L.stride; ctx->bpar = a + L.par;
        ctx->bn = (int)n; ctx->stream = st;
    };
    ctx->have_theta = true;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = B - b0 < chunk ? B - b0 : chunk;
        for (int64_t b = 0; b < nb; b++) {
            const double* th = thetas + (b0 + b) * w;
            double* row = hpar + b * GPRY_BPAR_ROW;
            for (int k = 0; k <= GPRY_MAX_DIM; k++) row[k] = 1.0;
            row[0] = exp(th[0]);                                     // as make_kp / make_ap for one evaluation
            for (int k = 0; k < ctx->d; k++) row[1 + k] = exp(th[1 + k]);
            row[GPRY_BPAR_WHITE] = ctx->white ? exp(th[1 + ctx->d]) : 0.0;
            objective_row_unwritten(hres + b * GPRY_BRES_STRIDE, bc.info_at);
        }
        for (int k = 0; k < w; k++) ctx->theta[k] = thetas[b0 * w + k];      // (the launchers read the sizes, not these, in a batch)
        // test hook ("panel_debug" bit 7): every scratch set starts as NaNs -- a result that depended on what a set held before shows
        if (ctx->opt_panel_debug & 128) HIP_TRY(ctx, hipMemsetAsync(a0, 0xFF, sizeof(double) * (size_t)(nb * L.stride), main_stream));
        HIP_TRY(ctx, hipMemcpy2DAsync(a0 + L.par, sizeof(double) * L.stride, hpar, sizeof(double) * GPRY_BPAR_ROW,
                                      sizeof(double) * GPRY_BPAR_ROW, (size_t)nb, hipMemcpyHostToDevice, main_stream));
        // Stream groups (throughput schedule): the panel chain of the Cholesky is one workgroup's latency per step whatever the
        // number of thetas, and between two products of a group the GPU drains.  With the thetas dealt over G streams the host
        // queues group after group; the groups run out of step by themselves and one's panel steps sit underneath the others' GEMMs.
        int G = 1;
        if (tp) { G = ctx->opt_lml_streams; if (G > nb) G = (int)nb; if (G < 1) G = 1; }
        if (G > 1) {
            while ((int)ctx->tp_streams.size() < G - 1) {
                hipStream_t st;
                HIP_TRY(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
                ctx->tp_streams.push_back(st);
            }
            while ((int)ctx->tp_events.size() < G) {
                hipEvent_t ev;
                HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                ctx->tp_events.push_back(ev);
            }
            HIP_TRY(ctx, hipEventRecord(ctx->tp_events[0], main_stream));        // the parameters are on the device
        }
        {
            StageScope s(ctx, bc.name, main_stream);
            int64_t t0 = 0;
            int rc = 0;
            for (int g = 0; g < G && rc == 0; g++) {
                const int64_t n = nb / G + (g < nb % G ? 1 : 0);
                const hipStream_t st = g == 0 ? main_stream : ctx->tp_streams[(size_t)g - 1];
                if (g > 0) {
                    const hipError_t e = hipStreamWaitEvent(st, ctx->tp_events[0], 0);
                    if (e != hipSuccess) { rc = gpry_fail(ctx, -2, "%s: %s", bc.name, hipGetErrorString(e)); break; }
                }
                point_at(t0, n, st);
                rc = bc.chain(ctx, want_grad, static_cast<double*>(ctx->hbres_dev) + t0 * GPRY_BRES_STRIDE);
                t0 += n;
            }
            // the main stream joins the groups (also on the error path: nothing of this call may still be in flight afterwards)
            for (int g = 1; g < G; g++) {
                const hipStream_t st = ctx->tp_streams[(size_t)g - 1];
                if (hipEventRecord(ctx->tp_events[(size_t)g], st) != hipSuccess || hipStreamWaitEvent(main_stream, ctx->tp_events[(size_t)g], 0) != hipSuccess)
                    (void)hipStreamSynchronize(st);
            }
            ctx->stream = main_stream;
            if (rc) { (void)hipStreamSynchronize(main_stream); return rc; }
        }
        HIP_TRY(ctx, hipStreamSynchronize(main_stream));
        for (int64_t b = 0; b < nb; b++) {
            const double* o = hres + b * GPRY_BRES_STRIDE;
            int inf = 0;
            GPRY_TRY(objective_status(ctx, bc.name, b0 + b, o, bc.info_at, &inf));
            if (info) info[b0 + b] = inf;
            objective_write(ctx, inf, bc.value(o), o + bc.head, nullptr, lml + b0 + b, want_grad ? grad + (b0 + b) * w : nullptr, nullptr);
        }
    }
    return 0;
}

__global__ void zero_upper_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int64_t n) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    int64_t i = idx / n, j = idx - i * n;
    dst[idx] = (j <= i) ? src[i * ld + j] : 0.0;
}

extern "C" {

int gpry_kernel_train(gpry_ctx* ctx, int add_alpha, double* K_out) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kernel_train: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, false));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GPRY_TRY(launch_scale_train(ctx));
    ctx->lml_cache = false;      // dW is about to be overwritten
    {
        StageScope s(ctx, "kernel_build");
        GPRY_TRY(launch_kernel_train(ctx, ctx->dW, add_alpha));
    }
    if (K_out) GPRY_TRY(copy_out_matrix(ctx, ctx->dW, ctx->Np, ctx->N, ctx->N, K_out));
    else HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int gpry_kernel_cross(gpry_ctx* ctx, const double* Xc_, int64_t M, double* K_out) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kernel_cross: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, false));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M <= 0) return 0;
    int64_t mp = round_up(M, 256);
    TmpBuf<double> bX, bK;
    GPRY_TRY(bX.alloc(ctx, M * ctx->d));
    GPRY_TRY(bK.alloc(ctx, ctx->Np * mp));
    double *dX = bX.p, *dK = bK.p;
    HIP_TRY(ctx, hipMemcpyAsync(dX, Xc_, sizeof(double) * M * ctx->d, hipMemcpyHostToDevice, ctx->stream));
    GPRY_TRY(launch_scale_train(ctx));
    int64_t saveM = ctx->sw_M; ctx->sw_M = M;
    int rc = launch_cross_build(ctx, dX, 0, mp, mp, dK, nullptr, 0);
    ctx->sw_M = saveM;
    if (rc) return rc;
    // dK is N x mp (k-major); the caller wants M x N: transpose on the host side copy
    std::vector<double> tmp((size_t)ctx->N * M);
    GPRY_TRY(copy_out_matrix(ctx, dK, mp, ctx->N, M, tmp.data()));
    for (int64_t j = 0; j < ctx->N; j++)
        for (int64_t m = 0; m < M; m++) K_out[m * ctx->N + j] = tmp[(size_t)j * M + m];
    return 0;
}

int gpry_factorize(gpry_ctx* ctx, int* info) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_factorize: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, false));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->factor_valid = false;
    ctx->kb_n = 0;
    int inf = 0;
    // The optimiser's last objective evaluation is normally at the theta it returns: its factor
    // (L in dW, V in dW2; same kernels, same inputs => the bits a fresh factorisation would give)
    // is adopted by swapping buffers instead of factorising again.
    bool hit = ctx->opt_lml_cache && ctx->lml_cache && ctx->lml_kernel_id == (ctx->kernel_id | (ctx->white ? GPRY_KERNEL_WHITE : 0));
    for (int k = 0; hit && k < ctx_ntheta(ctx); k++) hit = ctx->lml_theta[k] == ctx->theta[k];
    ctx->lml_cache = false;
    if (hit) {
        std::swap(ctx->dA, ctx->dW);
        std::swap(ctx->dV, ctx->dW2);
        GPRY_TRY(launch_scale_train(ctx));
    } else {
        GPRY_TRY(build_factor(ctx, ctx->dA, ctx->dV, ctx->dW, &inf));
    }
    if (info) *info = inf;
    if (inf != 0) return 0;
    // alpha_ = V^T (V y)
    GPRY_TRY(solve_alpha(ctx, ctx->dV, ctx->dy, ctx->dvec, ctx->dalpha_, ctx->Np));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->factor_valid = true;
    ctx->alpha_l2 = -1.0;
    return 0;
}

int gpry_get_factor(gpry_ctx* ctx, double* L, double* V, double* alpha_) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_get_factor: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int64_t N = ctx->N;
    if (L) {
        TmpBuf<double> bt;
        GPRY_TRY(bt.alloc(ctx, N * N));
        double* tmp = bt.p;
        hipLaunchKernelGGL(zero_upper_copy_kernel, dim3((unsigned)((N * N + 255) / 256)), dim3(256), 0,
                           ctx->stream, ctx->dA, tmp, ctx->Np, N);
        HIP_TRY(ctx, hipMemcpyAsync(L, tmp, sizeof(double) * N * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (V) GPRY_TRY(copy_out_matrix(ctx, ctx->dV, ctx->Np, N, N, V));
    if (alpha_) {
        HIP_TRY(ctx, hipMemcpyAsync(alpha_, ctx->dalpha_, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int gpry_lml(gpry_ctx* ctx, const double* theta, int want_grad, double* lml, double* grad, int* info) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_lml: ctx is NULL");
    if (!theta || !lml || (want_grad && !grad)) return gpry_fail(ctx, -1, "lml: theta, lml and (with want_grad) grad must not be NULL");
    GPRY_TRY(objective_entry(ctx, "lml", theta, 1));
    double *hres, *dres;
    GPRY_TRY(objective_row(ctx, 4096, RES_INFO, &hres, &dres));
    ThetaScope at(ctx, theta);
    // N <= 128, d <= 16: the whole evaluation in one launch of one workgroup (lml_small.hip); it leaves no factor in
    // dW / dW2 and does not touch the scaled coordinates of the prediction factor
    bool fused = false;
    double fhost[2 + GPRY_THETA_MAX];
    int rc = 0, inf = 0;
    if (ctx->opt_lml_small && ctx->opt_chol == 0) {
        StageScope s(ctx, "lml_small");
        const int r = launch_lml_small(ctx, want_grad, fhost, &inf);     // returns with the results in hand
        if (r < 0) rc = r;
        fused = r == 0;
    }
    if (!fused) {
        if (rc == 0) {
            rc = lml_chain(ctx, want_grad, dres);
            at.factor_chain_ran();      // (an optimiser's next evaluation does not need the coordinates put back)
        }
        rc = objective_wait(ctx, "lml", rc, hres, RES_INFO, &inf);
    }
    // the chain left L in dW and V in dW2: gpry_factorize at this theta adopts them
    ctx->lml_cache = rc == 0 && inf == 0 && !fused;
    if (ctx->lml_cache) {
        memset(ctx->lml_theta, 0, sizeof(ctx->lml_theta));
        for (int k = 0; k < ctx_ntheta(ctx); k++) ctx->lml_theta[k] = theta[k];
        ctx->lml_kernel_id = ctx->kernel_id | (ctx->white ? GPRY_KERNEL_WHITE : 0);
    }
    if (rc) return rc;
    if (info) *info = inf;
    const double* row = fused ? fhost : hres;
    objective_write(ctx, inf, lml_head(row), row + 2, nullptr, lml, want_grad ? grad : nullptr, nullptr);
    return 0;
}

// B objective evaluations in one call: the optimiser runs of a multi-restart fit stepped side by side (gpry/gpr.py:883-994 runs
// them one after another).  N <= 128, d <= 16: ONE launch, one workgroup per theta (lml_small.hip); up to Np = lml_batch
// (default 4096): ONE chain of launches for all thetas (objective_batch_general) -- either way every theta gets the arithmetic of a
// single gpry_lml call, hence the same bits; otherwise the thetas are evaluated one after another.
int gpry_lml_batch(gpry_ctx* ctx, const double* thetas, int64_t B, int want_grad, double* lml, double* grad, int* info) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_lml_batch: ctx is NULL");
    if (B <= 0) return 0;
    if (!thetas || !lml || (want_grad && !grad)) return gpry_fail(ctx, -1, "lml_batch: thetas, lml and (with want_grad) grad must not be NULL");
    GPRY_TRY(objective_entry(ctx, "lml_batch", thetas, B));
    const int w = ctx_ntheta(ctx);
    const bool fused = ctx->opt_lml_small && ctx->opt_chol == 0 && ctx->Np == 128 && ctx->d <= 16 && B <= 256;
    // (throughput schedule: a single theta goes through the chain of the many as well -- its result must not depend on B)
    if (!fused && (B >= 2 || ctx->opt_lml_schedule == 1) && lml_batch_usable(ctx)) {
        const int r = objective_batch_general(ctx, LML_BATCH, thetas, B, want_grad, lml, grad, info);
        if (r <= 0) return r;               // 1: no room for two sets, one after another below
    }
    if (!fused) {
        for (int64_t b = 0; b < B; b++) {
            int inf = 0;
            GPRY_TRY(gpry_lml(ctx, thetas + b * w, want_grad, lml + b, want_grad ? grad + b * w : nullptr, &inf));
            if (info) info[b] = inf;
        }
        return 0;
    }
    std::vector<double> par((size_t)B * 18, 1.0), out((size_t)B * (2 + 1 + GPRY_MAX_DIM), 0.0);
    std::vector<int> inf((size_t)B, 0);
    for (int64_t b = 0; b < B; b++) {
        par[b * 18] = exp(thetas[b * w]);                                   // as make_kp / make_ap for one evaluation
        for (int k = 0; k < ctx->d; k++) par[b * 18 + 1 + k] = exp(thetas[b * w + 1 + k]);
        par[b * 18 + 17] = ctx->white ? exp(thetas[b * w + 1 + ctx->d]) : 0.0;
    }
    {
        StageScope s(ctx, "lml_small");
        const int r = launch_lml_small_batch(ctx, (int)B, par.data(), want_grad, out.data(), inf.data());
        if (r < 0) return r;
        if (r != 0) return gpry_fail(ctx, -1, "lml_batch: the model does not fit the single-launch kernel");
    }
    for (int64_t b = 0; b < B; b++) {
        const double* o = out.data() + b * (2 + 1 + GPRY_MAX_DIM);
        if (info) info[b] = inf[b];
        objective_write(ctx, inf[b], lml_head(o), o + 2, nullptr, lml + b, want_grad ? grad + b * w : nullptr, nullptr);
    }
    return 0;
}

}  // extern "C"

// gpry_predict works on its own candidate set: swap it in for the duration of the call
struct PredictSetGuard {
    gpry_ctx* c;
    explicit PredictSetGuard(gpry_ctx* ctx) : c(ctx) { swap(); }
    ~PredictSetGuard() { swap(); }
    void swap() {
        std::swap(c->sw_M, c->pr.M); std::swap(c->sw_cap, c->pr.cap);
        std::swap(c->dXc, c->pr.dXc); std::swap(c->dmask, c->pr.dmask);
        std::swap(c->dy_all, c->pr.dy); std::swap(c->dsig_all, c->pr.dsig);
        std::swap(c->dacq_all, c->pr.dacq);
    }
};

extern "C" {

int gpry_predict(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask, double* mean, double* std) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict: ctx is NULL");
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M <= 0) return 0;
    if (!X) return gpry_fail(ctx, -1, "predict: X is NULL");
    if (!std && M <= GPRY_SERVE_MAXM && ctx->opt_predict_serve && ctx->opt_predict_small > 0) {
        // Latency path of the point-by-point callers (gpry/gp_acquisition.py:766-771, gpry/mc.py:387-391): no kernel
        // launch, the request goes to the resident kernel (server.hip) -- same slices, same sums, same bits as the
        // one-launch path below.
        double part[GPRY_SERVE_MAXM * 8];
        unsigned gbits[GPRY_SERVE_MAXM];
        int nsplit = 1;
        GPRY_TRY(serve_predict_mean(ctx, X, M, part, &nsplit, gbits));
        for (int64_t m = 0; m < M; m++) {
            double mu_ = 0.0;
            for (int sidx = 0; sidx < nsplit; sidx++) mu_ += part[m * nsplit + sidx];
            double y = fmin(mu_ * ctx->tf.y_std + ctx->tf.y_mean, ctx->tf.clip_hi);
            if ((mask && mask[m]) || gbits[m]) y = -INFINITY;
            mean[m] = y;
        }
        return 0;
    }
    GPRY_TRY(serve_stop(ctx));
    // "predict_gates" = 1: the verdicts of gpry_set_gates are ORed into the caller's mask here as gpry_sweep_logexp
    // does (the small paths below post-process on the host: they get a merged host mask; the panel paths run the
    // gates kernel on their resident candidate buffers)
    const bool dev_gates = ctx->gates_on && ctx->opt_predict_gates;
    std::vector<uint8_t> merged;
    if (dev_gates && M <= 4096) {
        const int64_t xb = round_up(sizeof(double) * M * ctx->d, 256);
        GPRY_TRY(ensure_pinned(ctx, xb + round_up(M, 256)));
        char* h = (char*)ctx->hpin; char* hd = (char*)ctx->hpin_dev;
        memcpy(h, X, sizeof(double) * M * ctx->d);
        if (mask) memcpy(h + xb, mask, (size_t)M); else memset(h + xb, 0, (size_t)M);
        GPRY_TRY(launch_gates(ctx, (const double*)hd, M, (uint8_t*)(hd + xb)));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        merged.assign((uint8_t*)(h + xb), (uint8_t*)(h + xb) + M);
        mask = merged.data();
    }
    if (!std && M <= ctx->opt_predict_small) {   // (predict_small = 0 switches both small-batch paths off)
        // Latency path (samplers call this per point, gpry/gp_acquisition.py:769-793): the points,
        // the mask and the result live in one pinned host buffer that the kernel reads and
        // writes directly -- one launch and one stream synchronisation, no copies, no timers.
        // The training rows are split over up to 8 workgroups per point; the host adds the
        // slices in a fixed order and applies the affine map, the clip and the mask.
        int nsplit = (int)(ctx->N / 1024);
        if (nsplit < 1) nsplit = 1;
        if (nsplit > 8) nsplit = 8;
        const int64_t xb = round_up(sizeof(double) * M * ctx->d, 256);
        GPRY_TRY(ensure_pinned(ctx, xb + sizeof(double) * M * nsplit));
        char* h = (char*)ctx->hpin;
        char* hd = (char*)ctx->hpin_dev;           // the same buffer as the device sees it
        memcpy(h, X, sizeof(double) * M * ctx->d);
        double* hp = (double*)(h + xb);
        GPRY_TRY(launch_predict_mean_small(ctx, (const double*)hd, M, nsplit, (double*)(hd + xb)));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t m = 0; m < M; m++) {
            double mu_ = 0.0;
            for (int sidx = 0; sidx < nsplit; sidx++) mu_ += hp[m * nsplit + sidx];
            double y = fmin(mu_ * ctx->tf.y_std + ctx->tf.y_mean, ctx->tf.clip_hi);
            if (mask && mask[m]) y = -INFINITY;
            mean[m] = y;
        }
        return 0;
    }
    if (std && M <= 4 && ctx->opt_predict_small > 0) {
        // a handful of points with std: k* rows + one multi-vector triangular product; partial sums come
        // back through pinned memory.  54 us for one point at N = 4096 and ~16 us per further point; from
        // five points on the split-K contraction below (138 us for up to 128 points) is faster
        const int64_t Np = ctx->Np, nmb = (Np + 255) / 256, nsb = Np / 16;
        const int64_t xb = round_up(sizeof(double) * M * ctx->d, 256);
        GPRY_TRY(ensure_pinned(ctx, xb + sizeof(double) * M * (nmb + nsb)));
        if (M * Np > ctx->g_cap) {
            if (ctx->dG) GPRY_TRY(dev_free(ctx, ctx->dG));
            ctx->dG = nullptr; ctx->g_cap = 0;
            GPRY_TRY(dev_alloc(ctx, &ctx->dG, 16 * Np));
            ctx->g_cap = 16 * Np;
        }
        char* h = (char*)ctx->hpin;
        char* hd = (char*)ctx->hpin_dev;           // the same buffer as the device sees it
        memcpy(h, X, sizeof(double) * M * ctx->d);
        double* hm = (double*)(h + xb);
        double* hs = hm + M * nmb;
        GPRY_TRY(launch_predict_small_std(ctx, (const double*)hd, (int)M, ctx->dG, (double*)(hd + xb),
                                          (double*)(hd + xb) + M * nmb));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const double C = ctx_prior_var(ctx);       // C + w for a model with a white term
        for (int64_t m = 0; m < M; m++) {
            double mu_ = 0.0, ss = 0.0;
            for (int64_t b = 0; b < nmb; b++) mu_ += hm[m * nmb + b];
            for (int64_t b = 0; b < nsb; b++) ss += hs[m * nsb + b];
            double y = fmin(mu_ * ctx->tf.y_std + ctx->tf.y_mean, ctx->tf.clip_hi);
            unsigned mk = mask ? mask[m] : 0u;
            if (mk) y = -INFINITY;
            mean[m] = y;
            double var = C - ss;
            if (var < 0.0) var = 0.0;
            double sd = sqrt(var) * ctx->tf.y_std;
            if (mk & GPRY_MASK_CLASSIFIED_INF) sd = 0.0;
            std[m] = sd;
        }
        return 0;
    }
    PredictSetGuard guard(ctx);
    SweepRequest rq;
    rq.kind = SWEEP_PREDICT; rq.have_mask = mask != nullptr; rq.want_std = std != nullptr;
    if (M <= 4096) {
        // A few thousand points: candidates, mask and results live in the pinned, device-mapped staging
        // buffer that the kernels read and write directly.  Four pageable hipMemcpyAsync calls cost more
        // (~100 us together) than the whole contraction of such a batch.
        const int64_t xb = round_up(sizeof(double) * M * ctx->d, 256), mb = round_up(M, 256), ob = round_up(sizeof(double) * M, 256);
        GPRY_TRY(ensure_pinned(ctx, xb + mb + 3 * ob));
        char* h = (char*)ctx->hpin;
        char* hd = (char*)ctx->hpin_dev;
        memcpy(h, X, sizeof(double) * M * ctx->d);
        if (mask) memcpy(h + xb, mask, (size_t)M);
        struct Saved { double* X; uint8_t* m; double *y, *s, *a; int64_t cap; } sv =
            {ctx->dXc, ctx->dmask, ctx->dy_all, ctx->dsig_all, ctx->dacq_all, ctx->sw_cap};
        ctx->dXc = (double*)hd; ctx->dmask = (uint8_t*)(hd + xb);
        ctx->dy_all = (double*)(hd + xb + mb); ctx->dsig_all = (double*)(hd + xb + mb + ob);
        ctx->dacq_all = (double*)(hd + xb + mb + 2 * ob);
        int rc = run_sweep(ctx, M, rq);
        hipError_t e = hipStreamSynchronize(ctx->stream);
        ctx->dXc = sv.X; ctx->dmask = sv.m; ctx->dy_all = sv.y; ctx->dsig_all = sv.s; ctx->dacq_all = sv.a; ctx->sw_cap = sv.cap;
        ctx->sw_M = 0;                       // the staging buffer is not a resident candidate set
        if (rc) return rc;
        if (e != hipSuccess) return gpry_fail(ctx, -2, "predict: %s", hipGetErrorString(e));
        memcpy(mean, h + xb + mb, sizeof(double) * M);
        if (std) memcpy(std, h + xb + mb + ob, sizeof(double) * M);
        return 0;
    }
    GPRY_TRY(upload_candidates(ctx, X, M, mask));
    if (dev_gates) {
        if (!rq.have_mask) HIP_TRY(ctx, hipMemsetAsync(ctx->dmask, 0, (size_t)M, ctx->stream));
        GPRY_TRY(launch_gates(ctx, ctx->dXc, M, ctx->dmask));
        rq.have_mask = true;
    }
    GPRY_TRY(run_sweep(ctx, M, rq));
    HIP_TRY(ctx, hipMemcpyAsync(mean, ctx->dy_all, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->stream));
    if (std) HIP_TRY(ctx, hipMemcpyAsync(std, ctx->dsig_all, sizeof(double) * M, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int gpry_predict_grad(gpry_ctx* ctx, const double* x, int want_kinv, double* kgrad, double* mean_grad,
                      double* kinvk_grad) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_grad: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, want_kinv || mean_grad != nullptr));   // kgrad alone needs no factor
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!x) return gpry_fail(ctx, -1, "predict_grad: x is NULL");
    const int64_t Np = ctx->Np;
    const int dpad = ctx->dpad, d = ctx->d;
    if (Np * dpad > ctx->g_cap) {
        if (ctx->dG) GPRY_TRY(dev_free(ctx, ctx->dG));
        ctx->dG = nullptr; ctx->g_cap = 0;
        GPRY_TRY(dev_alloc(ctx, &ctx->dG, Np * dpad));
        ctx->g_cap = Np * dpad;
    }
    if (!ctx->factor_valid) GPRY_TRY(launch_scale_train(ctx));   // scaled rows are normally made by the factorisation
    if (want_kinv) GPRY_TRY(ensure_part(ctx, (Np / 128) * Np));
    double* kstar = ctx->dvec; double* u = ctx->dvec + Np; double* w = ctx->dvec + 2 * Np;
    double* out = ctx->dvec + 3 * Np; double* xdev = out + 2 * GPRY_MAX_DIM;
    HIP_TRY(ctx, hipMemcpyAsync(xdev, x, sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
    {
        StageScope s(ctx, "predict_grad");
        GPRY_TRY(launch_gradx(ctx, xdev, 1, want_kinv, kstar, ctx->dG, u, w, ctx->dpart, out));
    }
    double h[2 * GPRY_MAX_DIM];
    HIP_TRY(ctx, hipMemcpyAsync(h, out, sizeof(double) * 2 * dpad, hipMemcpyDeviceToHost, ctx->stream));
    if (kgrad) GPRY_TRY(copy_out_matrix(ctx, ctx->dG, dpad, ctx->N, d, kgrad));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < d; k++) {
        if (mean_grad) mean_grad[k] = h[k];
        if (kinvk_grad) kinvk_grad[k] = want_kinv ? h[dpad + k] : 0.0;
    }
    return 0;
}

// ONE point: posterior mean, std and the two x-gradient contractions in one call (what GaussianProcessRegressor.predict
// with return_mean_grad / return_std_grad asks for, once per L-BFGS step of the acquisition optimiser).  Mean and std are
// finalised as by gpry_predict (affine map of y, clipping, mask bits); the gradients are the raw contractions of
// gpry_predict_grad.
int gpry_predict_point(gpry_ctx* ctx, const double* x, int mask_bits, int want_kinv, double* mean, double* std,
                       double* mean_grad, double* kinvk_grad, int* verdict) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_point: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!x || !mean || !std || !mean_grad || (want_kinv && !kinvk_grad))
        return gpry_fail(ctx, -1, "predict_point: x, mean, std, mean_grad and (with want_kinv) kinvk_grad must not be NULL");
    const int64_t Np = ctx->Np;
    const int dpad = ctx->dpad, d = ctx->d;
    if (Np * dpad > ctx->g_cap) {
        if (ctx->dG) GPRY_TRY(dev_free(ctx, ctx->dG));
        ctx->dG = nullptr; ctx->g_cap = 0;
        GPRY_TRY(dev_alloc(ctx, &ctx->dG, Np * dpad));
        ctx->g_cap = Np * dpad;
    }
    if (want_kinv) GPRY_TRY(ensure_part(ctx, (Np / 128) * Np));
    const int64_t nmb = (Np + 255) / 256, nsb = Np / 16;
    const int64_t xb = round_up((int64_t)sizeof(double) * GPRY_MAX_DIM, 256);
    GPRY_TRY(ensure_pinned(ctx, xb + (int64_t)sizeof(double) * (nmb + nsb + 2 * GPRY_MAX_DIM) + 256));
    char* h = (char*)ctx->hpin;
    char* hd = (char*)ctx->hpin_dev;
    memcpy(h, x, sizeof(double) * d);
    double* hm = (double*)(h + xb);
    double* hs = hm + nmb;
    double* ho = hs + nsb;
    double* dm = (double*)(hd + xb);
    // "predict_gates" = 1: the classifier / trust-box verdict of gpry_set_gates for this point, ORed into mask_bits (one more
    // small launch in the same stream; the host-side libsvm call it replaces costs 40 us per step of the optimiser)
    const bool dev_gates = ctx->gates_on && ctx->opt_predict_gates;
    uint8_t* hmask = (uint8_t*)(ho + 2 * GPRY_MAX_DIM);
    if (dev_gates) {
        hmask[0] = 0;
        GPRY_TRY(launch_gates(ctx, (const double*)hd, 1, (uint8_t*)(hd + ((char*)hmask - h))));
    }
    {
        StageScope s(ctx, "predict_point");
        GPRY_TRY(launch_point_full(ctx, (const double*)hd, want_kinv, ctx->dvec, ctx->dG, ctx->dvec + Np, ctx->dpart,
                                   dm, dm + nmb, dm + nmb + nsb));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (dev_gates) mask_bits |= hmask[0];
    if (verdict) *verdict = mask_bits;
    double mu_ = 0.0, ss = 0.0;
    for (int64_t b = 0; b < nmb; b++) mu_ += hm[b];
    for (int64_t b = 0; b < nsb; b++) ss += hs[b];
    double y = fmin(mu_ * ctx->tf.y_std + ctx->tf.y_mean, ctx->tf.clip_hi);
    if (mask_bits) y = -INFINITY;
    *mean = y;
    double var = ctx_prior_var(ctx) - ss;
    if (var < 0.0) var = 0.0;
    double sd = sqrt(var) * ctx->tf.y_std;
    if (mask_bits & GPRY_MASK_CLASSIFIED_INF) sd = 0.0;
    *std = sd;
    for (int k = 0; k < d; k++) {
        mean_grad[k] = ho[k];
        if (kinvk_grad) kinvk_grad[k] = want_kinv ? ho[dpad + k] : 0.0;
    }
    return 0;
}

// column sums of squares of U (Np x ld): ss[i] = |u_i|^2, one workgroup per column
__global__ __launch_bounds__(256) void colsumsq_kernel(const double* __restrict__ U, int64_t ld, int64_t nrow,
                                                       double* __restrict__ ss) {
    __shared__ double red[256];
    const int64_t i = blockIdx.x;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < nrow; j += 256) { const double u = U[j * ld + i]; acc = fma(u, u, acc); }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) ss[i] = red[0];
}

int gpry_predict_grad_batch(gpry_ctx* ctx, const double* X, int64_t m, int want_kinv, double* mean, double* std,
                            double* mean_grad, double* kinvk_grad) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_predict_grad_batch: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (m <= 0) return 0;
    if (!X || !mean_grad || (want_kinv && !kinvk_grad)) return gpry_fail(ctx, -1, "predict_grad_batch: X, mean_grad and (with want_kinv) kinvk_grad must not be NULL");
    if (m > 4096) return gpry_fail(ctx, -1, "predict_grad_batch: at most 4096 points per call (got %lld)", (long long)m);
    hipStream_t st = ctx->stream;
    const int64_t Np = ctx->Np, mp = round_up(m, 128);
    const int nt = (int)(Np / 128), d = ctx->d, dpad = ctx->dpad;
    const bool need_u = want_kinv || std != nullptr;
    // workspace: points | k* panel (Np x mp) | U | W | mean partials (nt x mp) | |u|^2 (mp) | gradients (m x 2 dpad)
    const bool small_build = mp <= 512;
    const int ntm = small_build ? 4 * nt : nt;      // mean partials per point
    const int64_t need = round_up(m * d, 2) + 3 * Np * mp + (int64_t)ntm * mp + mp + m * 2 * dpad;
    if (need > ctx->g_cap) {
        if (ctx->dG) GPRY_TRY(dev_free(ctx, ctx->dG));
        ctx->dG = nullptr; ctx->g_cap = 0;
        GPRY_TRY(dev_alloc(ctx, &ctx->dG, need));
        ctx->g_cap = need;
    }
    double* dXb = ctx->dG;
    double* Kst = dXb + round_up(m * d, 2);
    double* Um = Kst + Np * mp;
    double* Wm = Um + Np * mp;
    double* mpart = Wm + Np * mp;
    double* ss = mpart + (int64_t)ntm * mp;
    double* gout = ss + mp;
    // A few hundred points (the rounds of an acquisition optimiser's restarts): the points and the three small result arrays
    // live in the pinned, device-mapped staging buffer that the kernels read and write directly -- one pageable upload and
    // three pageable downloads cost 40 us of a 130-us call.
    const bool zero_copy = small_build;
    double *hx = nullptr, *hmz = nullptr, *hsz = nullptr, *hgz = nullptr;
    if (zero_copy) {
        const int64_t o1 = round_up(m * d, 32), o2 = o1 + round_up((int64_t)ntm * mp, 32), o3 = o2 + round_up(mp, 32);
        GPRY_TRY(ensure_pinned(ctx, (int64_t)sizeof(double) * (o3 + m * 2 * dpad + 32)));
        double* hb = (double*)ctx->hpin;
        double* db = (double*)ctx->hpin_dev;
        hx = hb; hmz = hb + o1; hsz = hb + o2; hgz = hb + o3;
        memcpy(hx, X, sizeof(double) * m * d);
        dXb = db; mpart = db + o1; ss = db + o2; gout = db + o3;
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(dXb, X, sizeof(double) * m * d, hipMemcpyHostToDevice, st));
    }
    StageScope scope(ctx, "predict_grad_batch");
    const int64_t saveM = ctx->sw_M; ctx->sw_M = m;
    int rc = small_build ? launch_cross_build_small(ctx, dXb, 0, mp, mp, Kst, mpart, 1)
                         : launch_cross_build(ctx, dXb, 0, mp, mp, Kst, mpart, 1);
    ctx->sw_M = saveM;
    if (rc) return rc;
    auto splits = [&](int64_t tiles) { int n = 1; while (n < 16 && tiles * n * 2 <= 1024 && Np / (n * 2) >= 64) n *= 2; return n; };
    if (need_u) {       // U = V K*^T
        GemmArgs g = {};
        g.A = ctx->dV; g.lda = Np; g.B = Kst; g.ldb = mp; g.C = Um; g.ldc = mp;
        g.M = (int)Np; g.N = (int)mp; g.K = (int)Np; g.kmode = KM_A_LOWER; g.tile_map = TM_ROWMAJOR;
        g.nsplit = splits((int64_t)nt * (mp / 128));
        if (g.nsplit > 1) { GPRY_TRY(gemm_split_scratch(ctx, g.nsplit, Np * mp, &g.split_buf)); g.split_stride = Np * mp; }
        GPRY_TRY(gemm_f64_launch(ctx, g, false, false, EPI_STORE));
        hipLaunchKernelGGL(colsumsq_kernel, dim3((unsigned)m), dim3(256), 0, st, Um, mp, Np, ss);
    }
    if (want_kinv) {    // W = V^T U = K^-1 K*^T
        GemmArgs g = {};
        g.A = ctx->dV; g.lda = Np; g.B = Um; g.ldb = mp; g.C = Wm; g.ldc = mp;
        g.M = (int)Np; g.N = (int)mp; g.K = (int)Np; g.kmode = KM_AT_LOWER; g.tile_map = TM_ROWMAJOR;
        g.nsplit = splits((int64_t)nt * (mp / 128));
        if (g.nsplit > 1) { GPRY_TRY(gemm_split_scratch(ctx, g.nsplit, Np * mp, &g.split_buf)); g.split_stride = Np * mp; }
        GPRY_TRY(gemm_f64_launch(ctx, g, true, false, EPI_STORE));
    }
    GPRY_TRY(launch_gradx_batch(ctx, dXb, m, 1, want_kinv ? Wm : nullptr, mp, gout));
    std::vector<double> hmv, hsv, hgv;
    const double *hm = hmz, *hs = hsz, *hg = hgz;
    if (!zero_copy) {
        hmv.resize((size_t)ntm * mp); hsv.resize((size_t)mp); hgv.resize((size_t)m * 2 * dpad);
        HIP_TRY(ctx, hipMemcpyAsync(hmv.data(), mpart, sizeof(double) * ntm * mp, hipMemcpyDeviceToHost, st));
        if (need_u) HIP_TRY(ctx, hipMemcpyAsync(hsv.data(), ss, sizeof(double) * mp, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(hgv.data(), gout, sizeof(double) * m * 2 * dpad, hipMemcpyDeviceToHost, st));
        hm = hmv.data(); hs = hsv.data(); hg = hgv.data();
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double C = ctx_prior_var(ctx);
    for (int64_t i = 0; i < m; i++) {
        if (mean) {
            double mu_ = 0.0;
            for (int t = 0; t < ntm; t++) mu_ += hm[(size_t)t * mp + i];
            mean[i] = fmin(mu_ * ctx->tf.y_std + ctx->tf.y_mean, ctx->tf.clip_hi);
        }
        if (std) {
            double var = C - hs[i];
            if (var < 0.0) var = 0.0;
            std[i] = sqrt(var) * ctx->tf.y_std;
        }
        for (int k = 0; k < d; k++) {
            mean_grad[i * d + k] = hg[(size_t)i * 2 * dpad + k];
            if (kinvk_grad) kinvk_grad[i * d + k] = want_kinv ? hg[(size_t)i * 2 * dpad + dpad + k] : 0.0;
        }
    }
    return 0;
}

int gpry_set_gates(gpry_ctx* ctx, const double* sv, const double* coef, int64_t n_sv, double gamma,
                   double intercept, int positive_is_finite, const double* trust_bounds) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_set_gates: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->d <= 0) return gpry_fail(ctx, -1, "set_gates before set_train");
    if (n_sv < 0 || (n_sv > 0 && (!sv || !coef))) return gpry_fail(ctx, -1, "set_gates: bad support vectors");
    if (n_sv > ctx->gate_sv_cap) {
        if (ctx->gate_sv) GPRY_TRY(dev_free(ctx, ctx->gate_sv));
        if (ctx->gate_coef) GPRY_TRY(dev_free(ctx, ctx->gate_coef));
        ctx->gate_sv = ctx->gate_coef = nullptr; ctx->gate_sv_cap = 0;
        const int64_t cap = round_up(n_sv, 256);
        GPRY_TRY(dev_alloc(ctx, &ctx->gate_sv, cap * GPRY_MAX_DIM));
        GPRY_TRY(dev_alloc(ctx, &ctx->gate_coef, cap));
        ctx->gate_sv_cap = cap;
    }
    if (!ctx->gate_trust) GPRY_TRY(dev_alloc(ctx, &ctx->gate_trust, 2 * GPRY_MAX_DIM));
    if (n_sv > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->gate_sv, sv, sizeof(double) * n_sv * ctx->d, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->gate_coef, coef, sizeof(double) * n_sv, hipMemcpyHostToDevice, ctx->stream));
    }
    if (trust_bounds)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->gate_trust, trust_bounds, sizeof(double) * 2 * ctx->d, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->gate_nsv = n_sv; ctx->gate_gamma = gamma; ctx->gate_intercept = intercept;
    ctx->gate_positive_finite = positive_is_finite; ctx->gate_has_trust = trust_bounds != nullptr;
    ctx->gates_on = (n_sv > 0 || trust_bounds != nullptr);
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// Kriging-believer session
__global__ void scale_rows_kernel(const double* __restrict__ X, int64_t m, int d, int dpad, int has_aff,
                                  const double* __restrict__ lo, const double* __restrict__ span,
                                  const double* __restrict__ ls, double* __restrict__ out) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * dpad) return;
    int64_t i = idx / dpad; int k = (int)(idx - i * dpad);
    double v = 0.0;
    if (k < d) {
        v = X[i * d + k];
        if (has_aff) v = (v - lo[k]) / span[k];
        v = v / ls[k];
    }
    out[idx] = v;
}
// one wave per row x: out_dot[x] = U[x].U[p] ; out_k[x] = C k(|xs_x - xs_p|)  (kb_gram.h)
__global__ __launch_bounds__(256) void kb_gram_kernel(const double* __restrict__ U, int64_t ldu, int64_t n, int64_t p,
                                                      int64_t Np, const double* __restrict__ Xkb, int dpad,
                                                      int kid, double C, double* __restrict__ out_dot,
                                                      double* __restrict__ out_k) {
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n) return;
    kb_gram_entry(U, ldu, x, p, Np, Xkb, dpad, kid, C, out_dot, out_k);
}
__global__ __launch_bounds__(256) void kb_var0_kernel(const double* __restrict__ U, int64_t ldu, int64_t first,
                                                      int64_t m, int64_t Np, double C, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= m) return;
    const double* ux = U + (first + x) * ldu;
    double s = 0.0;
    for (int64_t i = lane; i < Np; i += 64) s = fma(ux[i], ux[i], s);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[x] = C - s;
}

extern "C" {

int gpry_kb_reset(gpry_ctx* ctx) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kb_reset: ctx is NULL");
    GPRY_TRY(require_model(ctx, true));
    ctx->kb_n = 0;
    return 0;
}

int gpry_kb_register(gpry_ctx* ctx, const double* X, int64_t m, int64_t* first, double* var0) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kb_register: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (m <= 0) { if (first) *first = ctx->kb_n; return 0; }
    StageScope kb_scope(ctx, "kb_register");
    hipStream_t st = ctx->stream;
    const int64_t Np = ctx->Np;
    int64_t need = ctx->kb_n + round_up(m, 128);
    // rows registered earlier were written with the padded size of that time as their stride: every path that
    // changes Np (set_train, append_rows) ends the session, so a stride change can only meet an empty session
    if (ctx->kb_n > 0 && ctx->kb_ld < Np) return gpry_fail(ctx, -4, "kb_register: session rows have stride %lld, model needs %lld", (long long)ctx->kb_ld, (long long)Np);
    if (need > ctx->kb_cap || Np > ctx->kb_ld) {
        // (the row buffer used to be sized kb_cap x Np_at_allocation only: after the training set grew within
        // ctx->cap -- Np 1280 -> 1408, same buffers -- a session of ~900+ rows ran over its end)
        int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1024, need > ctx->kb_cap ? 2 * ctx->kb_cap : ctx->kb_cap));
        double *nU = nullptr, *nX = nullptr, *nO = nullptr;
        GPRY_TRY(dev_alloc(ctx, &nU, cap * Np));
        GPRY_TRY(dev_alloc(ctx, &nX, cap * ctx->dpad));
        GPRY_TRY(dev_alloc(ctx, &nO, 2 * cap));
        if (ctx->kb_n > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(nU, ctx->dU, sizeof(double) * ctx->kb_n * Np, hipMemcpyDeviceToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(nX, ctx->dXkb, sizeof(double) * ctx->kb_n * ctx->dpad, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctx->dU) GPRY_TRY(dev_free(ctx, ctx->dU));
        if (ctx->dXkb) GPRY_TRY(dev_free(ctx, ctx->dXkb));
        if (ctx->dkbout) GPRY_TRY(dev_free(ctx, ctx->dkbout));
        ctx->dU = nU; ctx->dXkb = nX; ctx->dkbout = nO; ctx->kb_cap = cap; ctx->kb_ld = Np;
    }
    const int64_t mp = round_up(m, 128);
    // stage the candidates, build their cross-kernel panel, then U^T = K*  V^T
    TmpBuf<double> bX, bpar;
    GPRY_TRY(bX.alloc(ctx, m * ctx->d));
    GPRY_TRY(bpar.alloc(ctx, 3 * GPRY_MAX_DIM));
    double *dX = bX.p, *dpar = bpar.p;
    HIP_TRY(ctx, hipMemcpyAsync(dX, X, sizeof(double) * m * ctx->d, hipMemcpyHostToDevice, st));
    double hpar[3 * GPRY_MAX_DIM];
    for (int k = 0; k < GPRY_MAX_DIM; k++) {
        hpar[k] = k < ctx->d ? ctx->tf.x_lo[k] : 0.0;
        hpar[GPRY_MAX_DIM + k] = k < ctx->d ? ctx->tf.x_span[k] : 1.0;
        hpar[2 * GPRY_MAX_DIM + k] = k < ctx->d ? exp(ctx->theta[1 + k]) : 1.0;
    }
    HIP_TRY(ctx, hipMemcpyAsync(dpar, hpar, sizeof(hpar), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((m * ctx->dpad + 255) / 256)), dim3(256), 0, st, dX, m,
                       ctx->d, ctx->dpad, ctx->tf.has_x_affine, dpar, dpar + GPRY_MAX_DIM, dpar + 2 * GPRY_MAX_DIM,
                       ctx->dXkb + ctx->kb_n * ctx->dpad);
    GPRY_TRY(dev_grow(ctx, &ctx->dKst, &ctx->kst_cap, Np * mp));
    int64_t saveM = ctx->sw_M; ctx->sw_M = m;
    int rc = mp <= 512 ? launch_cross_build_small(ctx, dX, 0, mp, mp, ctx->dKst, nullptr, 1)
                       : launch_cross_build(ctx, dX, 0, mp, mp, ctx->dKst, nullptr, 1);
    ctx->sw_M = saveM;
    if (rc) return rc;
    GemmArgs g = {};
    g.A = ctx->dKst; g.lda = mp;          // A(x, k) = Kst[k][x]
    g.B = ctx->dV; g.ldb = Np;            // B(k, i) = V[i][k]
    g.C = ctx->dU + ctx->kb_n * Np; g.ldc = Np;
    g.M = (int)mp; g.N = (int)Np; g.K = (int)Np;
    g.kmode = KM_B_UPPER; g.lower_only = 0; g.tile_map = TM_ROWMAJOR;
    {   // a shortlist is a few hundred points: 2 x Np/128 tiles, the longest walks all Np/16 slabs alone (0.8 ms
        // at Np = 4096): split the k-ranges so that the launch fills the GPU (as gpry_predict does, section 4.5)
        // The factor depends on Np ONLY: the conditioned variances must not depend on how many points were
        // registered together (a sharded pool merges a different number of shortlist points than one context
        // selects, and the proposals are compared bit for bit, tests/test_group_gpu.py).
        int ns = 1;
        while (ns < 8 && Np / (ns * 2) >= 256) ns *= 2;
        if (ns > 1) {
            GPRY_TRY(gemm_split_scratch(ctx, ns, mp * Np, &g.split_buf));
            g.nsplit = ns; g.split_stride = mp * Np;
        }
    }
    GPRY_TRY(gemm_f64_launch(ctx, g, true, true, EPI_STORE));
    if (var0) {
        hipLaunchKernelGGL(kb_var0_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, ctx->dU, Np, ctx->kb_n, m,
                           Np, ctx_prior_var(ctx), ctx->dkbout);      // (C + w for a model with a white term)
        HIP_TRY(ctx, hipMemcpyAsync(var0, ctx->dkbout, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (first) *first = ctx->kb_n;
    ctx->kb_n += m;
    return 0;
}

int gpry_kb_gram(gpry_ctx* ctx, int64_t p, double* G, double* kvec, int64_t* n) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kb_gram: ctx is NULL");
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (p < 0 || p >= ctx->kb_n) return gpry_fail(ctx, -1, "kb_gram: index %lld out of range [0, %lld)", (long long)p, (long long)ctx->kb_n);
    StageScope kb_scope(ctx, "kb_gram");
    hipStream_t st = ctx->stream;
    int64_t nn = ctx->kb_n;
    // the two result vectors go straight into the pinned, device-mapped staging buffer (no copy-out operations:
    // the ranking calls this once per accepted point, 15 times per cycle)
    GPRY_TRY(ensure_pinned(ctx, (int64_t)sizeof(double) * 2 * nn));
    double* hres = static_cast<double*>(ctx->hpin);
    double* dres = static_cast<double*>(ctx->hpin_dev);
    hipLaunchKernelGGL(kb_gram_kernel, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, st, ctx->dU, ctx->Np, nn, p,
                       ctx->Np, ctx->dXkb, ctx->dpad, ctx->kernel_id, exp(ctx->theta[0]), dres, dres + nn);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    memcpy(G, hres, sizeof(double) * nn);
    memcpy(kvec, hres + nn, sizeof(double) * nn);
    if (n) *n = nn;
    return 0;
}

}  // extern "C"

extern "C" int gpry_debug_gemm(gpry_ctx* ctx, const double* A, const double* B, double* C, int M, int N,
                               int K, int a_trans, int b_trans, int epi, int kmode, int lower_only,
                               int tile_map) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_debug_gemm: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    if (!A || !B || !C) return gpry_fail(ctx, -1, "debug_gemm: A, B and C must not be NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (M % 64 || N % 64 || K % 64) return gpry_fail(ctx, -1, "debug_gemm: dims must be multiples of 64");
    int64_t crow = (epi == EPI_SUMSQ) ? (M + 127) / 128 : M;
    TmpBuf<double> bA, bB, bC;
    GPRY_TRY(bA.alloc(ctx, (int64_t)M * K));
    GPRY_TRY(bB.alloc(ctx, (int64_t)K * N));
    GPRY_TRY(bC.alloc(ctx, crow * N));
    double *dA = bA.p, *dB = bB.p, *dC = bC.p;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(dA, A, sizeof(double) * M * K, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dB, B, sizeof(double) * K * N, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dC, C, sizeof(double) * crow * N, hipMemcpyHostToDevice, st));
    GemmArgs g = {};
    g.A = dA; g.lda = a_trans ? M : K;
    g.B = dB; g.ldb = b_trans ? K : N;
    g.C = dC; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.kmode = kmode; g.lower_only = lower_only; g.tile_map = tile_map & 0xff;
    g.small64 = (tile_map >> 28) & 1;             // test hook: bit 28 = eligible for the 64 x 64 tiles of gemm_small.hip
    const int nsplit = (tile_map >> 8) & 15;      // test hook: bits 8..11 of tile_map = split-K factor
    if (nsplit > 1) {
        GPRY_TRY(gemm_split_scratch(ctx, nsplit, (int64_t)crow * N, &g.split_buf));
        g.nsplit = nsplit; g.split_stride = (int64_t)crow * N;
    }
    const int seg = (tile_map >> 16) & 0xfff;     // test hook: bits 16..27 = stream-K segment length in slab pairs
    if (seg > 0) {
        if (M % 128 || N % 128 || K % 32) return gpry_fail(ctx, -1, "debug_gemm: stream-K needs M, N multiples of 128, K of 32");
        GemmPartsPlan pl;
        std::vector<GemmShape> sh = {{M, N, K}};
        GPRY_TRY(gemm_parts_plan_build(ctx, kmode, lower_only, sh, seg, &pl));
        int rc = gemm_dma_parts_launch(ctx, g, a_trans != 0, b_trans != 0, epi, pl, (int64_t)crow * N);
        if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = gpry_fail(ctx, -2, "debug_gemm: stream-K launch failed");
        gemm_parts_plan_free(&pl);
        if (rc) return rc;
    } else {
        StageScope s(ctx, "debug_gemm");
        GPRY_TRY(gemm_f64_launch(ctx, g, a_trans != 0, b_trans != 0, epi));
    }
    HIP_TRY(ctx, hipMemcpyAsync(C, dC, sizeof(double) * crow * N, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return 0;
}

// model-free entry to the acquisition epilogue of the sweep (the F5 edge vectors go through it)
extern "C" int gpry_debug_logexp(gpry_ctx* ctx, const double* mu, const double* sigma, int64_t n, double zeta,
                                 double baseline, double sigma_n, double* acq) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_debug_logexp: ctx is NULL");
    if (n <= 0) return 0;
    if (!mu || !sigma || !acq) return gpry_fail(ctx, -1, "debug_logexp: mu, sigma and acq must not be NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TmpBuf<double> bd;
    GPRY_TRY(bd.alloc(ctx, 3 * n));
    double* d = bd.p;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d, mu, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + n, sigma, sizeof(double) * n, hipMemcpyHostToDevice, st));
    GPRY_TRY(launch_logexp(ctx, d, d + n, n, zeta, baseline, sigma_n, d + 2 * n));
    HIP_TRY(ctx, hipMemcpyAsync(acq, d + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return 0;
}

