// Internal definitions shared by the gfx950 kernels behind include/gpry_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <map>

#include "../../include/gpry_hip.h"

#define GPRY_THETA_MAX (2 + GPRY_MAX_DIM)      // [log C, log l_1 .. l_d, log w]
#define GPRY_BPAR_ROW (2 + GPRY_MAX_DIM)       // parameter row of a batched evaluation: [C, l_1 .. l_32, w]
#define GPRY_BPAR_WHITE (1 + GPRY_MAX_DIM)
#define GPRY_TILE 128       // GEMM workgroup tile and padding quantum of N
#define GPRY_NB 64          // Cholesky / trtri base block

typedef double v4d __attribute__((ext_vector_type(4)));

struct StageTimer {
    double total_ms = 0.0;
    int64_t count = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// post-processing of a sweep's partial sums (sweep.hip: finish_y; acq_math.h: finish_sd, logexp_value)
struct FinishParams {
    double C, y_mean, y_std, clip_hi, zeta, baseline, sigma_n;
    int want_std, want_acq;
};

struct gpry_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;          // V = L^-1 phases of the pipelined factor chain run here, underneath potrf
    std::vector<hipEvent_t> ev_pool;        // one pair per Cholesky look-ahead step (never re-recorded within a call)
    char err[1024] = {0};

    // options
    int opt_chol = 0;
    int64_t opt_sweep_chunk = 0;         // 0: 32768 at Np >= 4096, proportionally more below (same panel bytes)
    int opt_timing = 0;          // per-stage HIP-event timers: off until gpry_timing_reset (or "timing" = 1) asks for them
    bool xs_foreign = false;     // dXs holds coordinates scaled for an LML evaluation's theta, not the prediction factor's (ensure_pred_xs)
    bool info_cleared = false;   // dinfo[0..3] were zeroed by launch_scale_train and nothing has touched them since
    int opt_gemm_small = 32;     // launches of at most this many 128 x 128 tiles run with 64 x 64 tiles (0: never)
    int64_t opt_predict_small = 2048;  // mean-only gpry_predict of at most this many points: one fused launch
    int opt_chol_overlap = 1;    // 1: trailing-update tiles ride in the panel launches (potrf_lower_overlap)

    // training set (transformed space)
    int64_t N = 0, Np = 0, cap = 0;  // cap: allocated padded size
    int d = 0, dpad = 0, dp_cap = 0;   // dp_cap: row width the X buffers were allocated for
    int kernel_id = GPRY_RBF;           // the stationary kernel alone (GPRY_KERNEL_WHITE is kept in `white`)
    bool white = false;                 // the model has a fitted white term w: theta[1 + d] = log w (ctx_white below)
    bool have_theta = false, factor_valid = false;
    double theta[GPRY_THETA_MAX] = {0};
    gpry_affine tf;
    // factor of the last successful gpry_lml evaluation: still sitting in dW (L) / dW2 (V)
    bool lml_cache = false;
    int lml_kernel_id = -1;             // (with the white flag)
    double lml_theta[GPRY_THETA_MAX] = {0};
    int opt_lml_cache = 1;
    unsigned long long lml_seq = 0;     // stamp of the last single-launch evaluation
    int opt_lml_small = 1;       // N <= 128, d <= 16: LML + gradient in one launch of one workgroup (lml_small.hip)

    // Batched objective above N = 128 (gpry_lml_batch, api.hip): the B thetas of a call go through ONE chain of launches.
    // Every kernel of the chain takes the theta index from blockIdx.z; the per-theta buffers (W, W2, W3, scaled
    // coordinates, vectors, partial sums, split-K slices, [C, l...], status words) are the same layout repeated
    // `bstride` doubles apart in one arena, so a kernel moves every per-theta pointer by the same number of bytes
    // (bset below).  Outside a batched evaluation bn = 1, bstride = 0, bpar = NULL and nothing changes.
    int bn = 1;
    int64_t bstride = 0;
    const double* bpar = nullptr;      // device, set 0: [C, l_1 .. l_d] as the host computes them for one evaluation, w at GPRY_BPAR_WHITE
    double* barena = nullptr; int64_t barena_cap = 0;     // doubles
    void* hbres = nullptr; void* hbres_dev = nullptr; int64_t hbres_cap = 0;   // results of a batch (pinned, device-mapped)
    int64_t opt_lml_batch = 4096;      // largest Np whose gpry_lml_batch runs as one chain (0: thetas one after another); measured
                                       // against the thread farm of three contexts: full fits 2.2x faster at N = 1024, 1.4x at 2048,
                                       // 1.1x at 4096, 0.9x at 8192 (tools/r04/time_fit_crossover.py, bench.py --workload farm)
    int64_t opt_lml_batch_mb = 49152;  // upper limit of the arena (MiB of the 288 GB): longer batches go through in chunks
    // Schedule of gpry_lml_batch (option "lml_schedule"): 0 = latency -- every theta gets the launches, and the bits, of a single
    // gpry_lml (stream-K / split-K partial sums, the inverse factor out of the Cholesky launches up to "chol_stacked"); 1 =
    // throughput -- the chain for MANY thetas at once: whole-tile products only (no partial slices to write and add), the
    // Cholesky in column blocks with one MFMA SYRK launch behind each, the thetas dealt over "lml_streams" streams so that one
    // group's panel chain runs underneath the other groups' products.  Its per-theta result does not depend on how many thetas
    // share the call (B = 1 included) and differs from the latency schedule's by rounding (another summation order).
    int opt_lml_schedule = 0;
    int opt_lml_streams = 2;           // throughput schedule: stream groups per call (1: one chain for all thetas)
    int64_t opt_tp_block = 512;        // throughput schedule: width of the column blocks of the Cholesky (multiple of 128)
    int opt_tp_left = 0;               // throughput schedule: 0 = the column blocks right-looking (one launch of the block's width behind each; default: measured ahead), 1 = left-looking (one deep launch in front of each); same bits
    int64_t opt_tp_tail = 1024;        // ... and the size of the last block, factored with riding tiles only
    int64_t batch_set_doubles = 0, batch_chunk = 0;     // the last batched evaluation's scratch set and thetas per chain (diagnostic, gpry_timing_get)
    int64_t batch_shrinks = 0;         // times a batched evaluation halved its chunk after an out-of-memory answer (diagnostic, gpry_timing_get "lml_batch_shrinks")
    int opt_chol_tp_segments = 0;      // 1: every factorisation of the context takes the column blocks of the throughput schedule (comparator: same bits)
    int opt_panel_debug = 0;           // ORed into GPRY_PANEL_FLAGS (chol_panel.hip); 64: the diagonal workgroup of every panel step reports a timed-out wait (test hook)
    bool tp = false;                   // a throughput-schedule chain is being queued (set by objective_batch_general only)
    std::vector<hipStream_t> tp_streams;   // the extra streams of the groups (created on first use)
    std::vector<hipEvent_t> tp_events;

    double* dX = nullptr;      // N x d raw transformed training rows (row-major, ld = d)
    double* dXs = nullptr;     // Np x dpad rows scaled by 1/l (pad rows = 0)
    double* dy = nullptr;      // Np
    double* dnoise = nullptr;  // Np (alpha = noise_^2; pad = 0)
    double* dA = nullptr;      // Np x Np : K then L (factor used for prediction)
    double* dV = nullptr;      // Np x Np : V = L^-1 (upper triangle exactly zero)
    double* dW = nullptr;      // Np x Np : scratch (lml: K/L ; T ; K^-1)
    double* dW2 = nullptr;     // Np x Np : scratch (lml: V)
    double* dW3 = nullptr;     // Np x Np : scratch (lml: T, then K^-1)
    double* dalpha_ = nullptr; // Np
    double* dvec = nullptr;    // small vectors / reductions (8 * Np + 4096 doubles)
    int* dinfo = nullptr;      // device status word(s)
    double* dparams = nullptr; // device copy of [C, 1/l..., lo..., span...] etc.

    // gates evaluated on the device inside gpry_sweep_logexp (gpry_set_gates)
    double* gate_sv = nullptr; double* gate_coef = nullptr; double* gate_trust = nullptr;
    int64_t gate_nsv = 0, gate_sv_cap = 0;
    double gate_gamma = 0.0, gate_intercept = 0.0;
    int gate_positive_finite = 1, gate_has_trust = 0, gates_on = 0;

    // sweep state
    int64_t sw_M = 0, sw_cap = 0;
    double* dXc = nullptr;     // M x d candidates (raw as given)
    uint8_t* dmask = nullptr;  // M
    double *dy_all = nullptr, *dsig_all = nullptr, *dacq_all = nullptr;  // M each
    // second candidate set, used by gpry_predict so that the resident NORA pool survives
    struct CandSet {
        int64_t M = 0, cap = 0;
        double* dXc = nullptr; uint8_t* dmask = nullptr;
        double *dy = nullptr, *dsig = nullptr, *dacq = nullptr;
    } pr;
    double* dXcs = nullptr;    // dsel x chunk: the candidates of the current chunk, scaled, coordinate-major (launch_cross_build)
    int64_t xcs_cap = 0;
    double* dYcs = nullptr;    // Np x dsel: centred scaled training rows of the MFMA panel build (launch_cross_prepare)
    int64_t ycs_cap = 0;
    double xcenter[GPRY_MAX_DIM] = {0};    // mean of the training rows per dimension: the centre both sides are shifted by
    double xsum[GPRY_MAX_DIM] = {0};       // its running sums, in row order (set_train, append_rows)
    double xlo[GPRY_MAX_DIM] = {0}, xhi[GPRY_MAX_DIM] = {0};     // smallest / largest training coordinate per dimension (error estimate of the MFMA panel)
    int opt_cross_mfma = 1;    // 1 (default): the sweep's cross-kernel panel takes its distances from the matrix pipe
    double alpha_l2 = -1.0;    // ||alpha_||_2 of the prediction factor (fetched when the panel form is chosen; < 0: not yet)
    double alpha_l1 = 0.0;     // ||alpha_||_1, fetched with it
    double noise_min = 0.0;    // smallest entry of the noise vector `alpha` of the training rows (set_train, append_rows): lambda_min(K) >= it + w
    int panel_form = 0;        // cross-kernel panel of the last sweep / panel predict: 0 none yet, 1 matrix pipe, 2 difference form, 3 small-batch kernel, 4 hybrid (matrix pipe, near pairs from the coordinates)
    int opt_cross_hybrid = 1;  // 1: a model that fails the gate of the matrix-pipe form because of SHORT length scales takes the hybrid form instead of the difference form
    double panel_est[4] = {0, 0, 0, 2.5e-7};   // its error estimates: mean (l2, gated), mean (l1, worst case), variance / C (gated), the gate
    double* dKst = nullptr;    // Np x chunk cross-kernel panel (k-major)
    int64_t kst_cap = 0;       // doubles allocated
    double* dG = nullptr;      // Np x dpad: d k(x, X_j)/dx of the last gpry_predict_grad
    int64_t g_cap = 0;
    double* dsplit = nullptr;  // split-K partial products of the factor GEMMs
    int64_t split_cap = 0;
    int opt_predict_split = 1; // split-K contraction for predict / sweeps of a few thousand points (one chunk)
    int opt_gemm_dma = 1;         // 128-aligned factor-chain products through gemm_dma_kernel
    double* dpart = nullptr;   // partial sums (sumsq per i-tile, mean per j-chunk)
    int64_t part_cap = 0;
    // top-k scratch
    unsigned long long* dkeys = nullptr; int64_t keys_cap = 0;
    unsigned int* dhist = nullptr;
    // "select_fused": 12 x 256 digit counters, one array per pass, and behind them the 12 SelState slots the passes hand on
    unsigned int* dselp = nullptr;
    enum { SELP_HIST_WORDS = 12 * 256, SELP_WORDS = 12 * 256 + 12 * 8 };
    int opt_select_fused = 1;          // 1: every select pass derives the previous pass's digit itself (no scan launches; sweep_topk.hip)
    int opt_prune_one_select = 1;      // 1: the first contraction round answers from its own records where these provably are the shortlist
    int opt_sweep_small_map = 1;       // 1: a one-pass contraction of at most 512 tiles launches one workgroup per tile, longest row tile first (sweep_gemm.hip)
    gpry_cand* dcand = nullptr; int64_t cand_cap = 0;
    unsigned long long* dsel = nullptr;  // DSEL_WORDS words: select state and the counters of the sweep
    enum { DSEL_NAN = 0,       // count_nan_kernel (between selections)
           DSEL_STATE = 0,     // SelState of a radix select, 4 words ...
           DSEL_EMIT = 4,      // ... and its two counters: records emitted, largest key below the threshold
           DSEL_SURV = 6,      // candidates whose bound is not below tau (prune_survivors)
           DSEL_GIDX = 7,      // indices written to dgidx
           DSEL_LIVE = 8,      // live blocks of the bound pass
           DSEL_FALL = 9,      // ... and, with its FP32 screen on, the blocks only the FP64 test skipped (the kernel takes DSEL_LIVE + 1)
           DSEL_WORDS = 64 };

    // Kriging-believer session
    int64_t kb_n = 0, kb_cap = 0;
    int64_t kb_ld = 0;         // row length dU was allocated for (Np may grow within ctx->cap: set_train, gpry_append_rows)
    double* dU = nullptr;      // kb_cap x kb_ld : row x = u(x)^T, used with stride Np <= kb_ld (x-major, contiguous u)
    double* dXkb = nullptr;    // kb_cap x dpad scaled candidate rows
    double* dkbout = nullptr;  // 2 * kb_cap

    double* dbord = nullptr;   // border workspace of gpry_append_rows: B, U (Np x 128), T (128 x Np), S / L22 / W22
    int64_t bord_cap = 0;
    int64_t n_border = 0;      // rows appended by border updates since the last full factorisation (diagnostic)

    void* trtri_plan = nullptr;
    void* trtri_pipe = nullptr;   // state of a pipelined factor chain in flight (chol.hip)
    int64_t opt_gemm_streamk = 5632;   // up to this Np the V = L^-1 levels >= 512 and K^-1 = V^T V are stream-K launches
                                       // (gemm_dma.hip; a gain up to 5120, neutral at 6144, a loss at 8192); 0 = off
    int64_t opt_topk_host = 16384;    // pools up to this size are selected on the host (gpry_sweep_topk)
    int opt_factor_pipeline = 1;  // 1: V = L^-1 phases run on stream2 underneath potrf
    int opt_factor_pipeline_min = 1280;   // from this Np on (ahead by 2-6% from 1280 up, level below: tools/r04/ab_pipeline_now.py)
    void* chol_plan = nullptr;    // cached tile schedule of the fused Cholesky (chol_panel.hip)   // cached batch descriptors of the V = L^-1 recursion (chol.hip)

    // resident predict kernel (server.hip)
    void* srv = nullptr;
    int opt_predict_serve = 1;         // mean-only gpry_predict of <= 8 points goes through the resident kernel
    int64_t opt_serve_idle_us = 2000;  // the kernel leaves after this long without a request
    int opt_mcmc_mapped = 0;           // gpry_mcmc_chains: 1 = the chains write their records to mapped pinned memory, 0 = to
                                       // device memory, copied back once per call (profiles/mcmc.md)
    int64_t opt_chol_stacked = 2048;   // up to this Np the inverse factor comes out of the Cholesky launches themselves (potrf_stacked, chol_panel.hip); 0: never
    int opt_chol_stacked_dense = 0;    // 1: potrf_stacked without use of the zero structure of the appended rows (comparator)
    int opt_sweep_overlap = 0;         // 1: the cross-kernel panel of chunk c + 1 is built on the side stream underneath the contraction of chunk c (two panels)
    int opt_sweep_upload = 1;          // 1: a fresh candidate pool is uploaded chunk by chunk on stream2, chunk c + 1 underneath the kernels of chunk c
    const double* up_X = nullptr;      // host pool of the sweep in flight whose chunks are still to be uploaded (sweep.hip: run_sweep)
    const double* up_y = nullptr;      // ... and the caller's y of a sweep with given y (gpry_sweep_logexp_given), beside them
    int up_gates = 0;                  // ... and the device gates are evaluated chunk by chunk behind each upload
    int opt_kb_rank = 1;               // 1: RankedPool.add ranks an offer through gpry_kb_rank (kb_rank.hip); 0: the Python path (the comparator)
    int opt_predict_gates = 0;         // 1: gpry_predict ORs the device gates (gpry_set_gates) into the caller's mask, as the sweep does
    // pruned sweep (option "sweep_prune", sweep.hip / sweep_topk.hip): gpry_sweep_logexp with no arrays wanted leaves y and a per-candidate upper
    // bound of the acquisition; gpry_sweep_topk contracts only the candidates whose bound can reach the shortlist
    int opt_sweep_prune = 0;
    // 1 (default): in the hybrid panel form, stage A of a pruned sweep bounds y instead of computing it (the bound pass,
    // sweep.hip: mean_bound_setup); exact y only for the candidates that are contracted
    int opt_sweep_mean_bound = 1;
    // 1 (default): the bound pass certifies far blocks with an FP32 screen in front of its FP64 test (kernel_build.hip: THE
    // SCREEN); 0: the FP64 test alone (the comparator: same skipped blocks, same outputs)
    int opt_sweep_screen = 1;
    int sw_pruned = 0;                 // 1: the resident sweep is pruned (acq_all holds exact values or bounds, see sweep_topk.hip)
    struct PruneState {
        int have_mask = 0;
        int form = 0;                  // panel form stage A decided (panel_form codes); compact panels take the same
        FinishParams fp = {};          // the model's post-processing the bounds were made with
        int64_t n_eval = 0;            // candidates evaluated exactly: the top n_eval by bound
        int64_t rounds = 0, evaluated_total = 0, completed = 0, last_K = 0;
        int64_t n_gidx = 0;            // candidates in dgidx (the last contracted set)
        int tau_done = 0;              // the survivor count of a threshold has been made (prune_survivors)
        double tau = 0.0;              // that threshold, and the candidates whose bound was not below it
        int64_t survivors = -1;
        int ybound = 0;                // stage A bounded y (the bound pass): every contraction computes y as well
        int64_t live_blocks = 0, blocks = 0;    // blocks of 16 training rows x 32 candidates the bound pass evaluated / saw
        int64_t cert_blocks = 0;                // ... and those its FP32 screen certified (gpry_sweep_screen_info)
    } prune;
    // the prediction state the pruned sweep was made with, copied at its end (sweep.hip: prune_snapshot): a later contraction
    // round or completion evaluates THAT model, whatever gpry_set_train / set_theta / factorize / append_rows did meanwhile
    struct ModelSnap {
        double *dV = nullptr, *dalpha_ = nullptr, *dXs = nullptr, *dX = nullptr;
        int64_t v_cap = 0, a_cap = 0, xs_cap = 0, x_cap = 0;
        int64_t N = 0, Np = 0;
        int d = 0, dpad = 0, kernel_id = 0;
        bool white = false;
        double theta[GPRY_THETA_MAX] = {0};
        gpry_affine tf;
        double xcenter[GPRY_MAX_DIM] = {0};
        bool xs_foreign = false;
    } snap;
    double* dub = nullptr;             // M: upper bound of each candidate's acquisition (prior sigma)
    int64_t ub_cap = 0;
    double* dXg = nullptr;             // gathered candidate rows of a compact evaluation (rows padded to 256, zeros)
    int64_t xg_cap = 0;                // doubles
    int64_t* dgidx = nullptr;          // their pool indices
    int64_t gidx_cap = 0;
    uint8_t* dmc = nullptr;            // gpry_mcmc_chains: start states, proposal factor and outputs (bytes)
    int64_t mc_cap = 0;
    // The call scratch (CallScratch below): the private device buffer of whichever entry point is running -- gpry_ns_knn,
    // gpry_ns_generation_phantoms, gpry_predict_cov / gpry_sample_joint, gpry_loo / gpry_leave_out, gpry_lml_hessian,
    // gpry_mean_theta_grad, gpry_predict_without, gpry_var_theta_grad, gpry_svm_fit.  Written and read between a call's
    // entry and its last stream synchronisation; no call reads what another left.
    uint8_t* dscratch = nullptr;       // bytes
    int64_t scratch_cap = 0, scratch_np = 0;    // ... and Np of the model when it last grew (ensure_capacity gives it back by that)
    const char* scratch_holder = nullptr;   // the entry point that holds it now (NULL: nobody)
    void* hloo = nullptr; int64_t hloo_cap = 0;    // gpry_loo: pinned landing place of its five output rows (bytes)
    void* hsvm = nullptr; int64_t hsvm_cap = 0;    // gpry_svm_fit: pinned image of its upload (bytes)
    int64_t opt_svm_iters = 4096;      // gpry_svm_fit: steps of one launch of the solver (the result does not depend on it)

    // host pinned staging
    void* hpin = nullptr; void* hpin_dev = nullptr; int64_t hpin_cap = 0;   // host / device view of the same buffer

    std::map<std::string, StageTimer> timers;
};

extern thread_local char g_last_error[1024];

// the white term of the model (GPRY_KERNEL_WHITE): w, the number of theta entries, the prior variance C + w of a new point
static inline double ctx_white(const gpry_ctx* ctx) { return ctx->white ? exp(ctx->theta[1 + ctx->d]) : 0.0; }
static inline int ctx_ntheta(const gpry_ctx* ctx) { return ctx->d + 1 + (ctx->white ? 1 : 0); }
static inline double ctx_prior_var(const gpry_ctx* ctx) {
    const double C = exp(ctx->theta[0]);
    return ctx->white ? C + exp(ctx->theta[1 + ctx->d]) : C;
}

int gpry_fail(gpry_ctx* ctx, int code, const char* fmt, ...);
// entry points that do not carry the white term yet: an error that names it, never a silently wrong variance
static inline int refuse_white(gpry_ctx* ctx, const char* who) {
    if (!ctx->white) return 0;
    return gpry_fail(ctx, -1, "%s: a model with a white term (WhiteKernel, GPRY_KERNEL_WHITE) is not supported by this entry point", who);
}

#define HIP_TRY(ctx, expr)                                                          \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess)                                                       \
            return gpry_fail(ctx, -2, "%s failed: %s (%s:%d)", #expr,               \
                             hipGetErrorString(_e), __FILE__, __LINE__);            \
    } while (0)

#define GPRY_TRY(expr)                 \
    do {                               \
        int _r = (expr);               \
        if (_r != 0) return _r;        \
    } while (0)

// scoped device timing of one stage on ctx->stream
struct StageScope {
    gpry_ctx* ctx; const char* name; hipEvent_t e0 = nullptr, e1 = nullptr; hipStream_t st = nullptr; bool marked = false;
    StageScope(gpry_ctx* c, const char* n, hipStream_t stream = nullptr);
    ~StageScope();
};
void timers_collect(gpry_ctx* ctx);

template <typename T>
int dev_alloc(gpry_ctx* ctx, T** p, int64_t count);
int dev_free(gpry_ctx* ctx, void* p);

static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// grow-only device buffer with one capacity (in elements): nothing to do while need <= *cap; else the stream is drained,
// the old buffer freed and `need` elements allocated (the contents are not kept)
template <typename T>
int dev_grow(gpry_ctx* ctx, T** p, int64_t* cap, int64_t need) {
    if (need <= *cap) return 0;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*p) GPRY_TRY(dev_free(ctx, *p));
    *p = nullptr; *cap = 0;
    GPRY_TRY(dev_alloc(ctx, p, need));
    *cap = need;
    return 0;
}

// The call scratch of the context (gpry_ctx::dscratch), held by one entry point at a time.  The caller names its regions
// with take<T>(count) -- they lie end to end on 256-byte boundaries, in the order taken -- then claim()s: an arena that
// somebody holds is an internal error (one claimant called another), else the buffer grows as dev_grow grows (stream
// drained, contents not kept).  at() gives a region's device pointer, NULL for a region of no elements.  The destructor
// lets go on every return path; what the holder queued on a side stream it has joined into ctx->stream by then, so the
// next holder's launches are ordered behind it by the stream.
struct CallScratch {
    template <class T> struct Reg { int i; };
    static const int CAP = 20;
    gpry_ctx* ctx; const char* who;
    int64_t bytes[CAP + 1], off[CAP + 1];      // (slot CAP: where a region beyond the capacity lands; claim() then fails)
    int n = 0; int64_t total = 0; bool held = false;

    CallScratch(gpry_ctx* c, const char* w) : ctx(c), who(w) {}
    ~CallScratch() { if (held) ctx->scratch_holder = nullptr; }
    template <class T> Reg<T> take(int64_t count) {
        const int i = n < CAP ? n : CAP;
        bytes[i] = (int64_t)sizeof(T) * count; off[i] = total;
        total += round_up(bytes[i], 256);
        n++;
        return {i};
    }
    int claim() {
        if (n > CAP) return gpry_fail(ctx, -1, "%s: %d scratch regions, the table holds %d", who, n, CAP);
        if (ctx->scratch_holder)
            return gpry_fail(ctx, -1, "%s: the call scratch is held by %s (internal error)", who, ctx->scratch_holder);
        if (total > ctx->scratch_cap) ctx->scratch_np = ctx->Np;
        GPRY_TRY(dev_grow(ctx, &ctx->dscratch, &ctx->scratch_cap, total));
        ctx->scratch_holder = who; held = true;
        return 0;
    }
    template <class T> T* at(Reg<T> h) const { return bytes[h.i] > 0 ? (T*)(ctx->dscratch + off[h.i]) : nullptr; }
};

// the buffer of theta `tb` in a batched launch (see gpry_ctx::bn): every per-theta pointer moves by tb * bstride doubles
// (pointer arithmetic, not integer arithmetic: the result keeps the provenance of a kernel argument, i.e. global loads
// and stores -- through an integer cast it became a flat pointer, and chol_fused_kernel went to scratch memory)
template <typename T>
__device__ __forceinline__ T* bset(T* p, int tb, int64_t bstride) {
    return (T*)((char*)p + (int64_t)tb * bstride * 8);
}
#define GPRY_BRES_STRIDE 40     // doubles per theta in the result buffer of a batch: [logdet/2, quad, grad (1 + 32), info0, info1]

// ---- GEMM (gemm_f64.hip) -----------------------------------------------------------
enum GemmKMode {
    KM_FULL = 0,      // k in [0, K)
    KM_A_LOWER = 1,   // A lower triangular (rows i, cols k): k < (ti+1)*TILE
    KM_B_LOWER = 2,   // B lower triangular (rows k, cols j): k >= tj*TILE
    KM_AT_LOWER_B_LOWER = 3, // C = A^T B with A, B lower: k >= max(ti, tj)*TILE
    KM_B_UPPER = 4,   // B upper triangular (rows k, cols j): k < (tj+1)*TILE
    KM_AT_LOWER = 5   // C = A^T B with A lower triangular (stored rows k, cols i): k >= ti*TILE
};
enum GemmEpi { EPI_STORE = 0, EPI_STORE_NEG = 1, EPI_SUB = 2, EPI_SUMSQ = 3 };
// TM_BALANCED (gemm_dma.hip): workgroups go to the XCDs round-robin by block index, so the enumeration
// decides the balance: tiles of equal k-length are neighbours (row-wise triangular order for lower-only
// square outputs, column-major where the length depends on the tile column), longest first
enum GemmTileMap { TM_ROWMAJOR = 0, TM_SWEEP = 1, TM_BALANCED = 2 };
// bit 12 of GemmArgs::tile_map, for sweep_gemm_dma_sp_launch alone: the small-launch map is allowed (option "sweep_small_map")
#define TM_SWEEP_SMALL (1 << 12)

struct GemmBatchItem { int64_t a_off, b_off, c_off; int M, N, K, pad; };

struct GemmArgs {
    const double* A; const double* B; double* C;
    int64_t lda, ldb, ldc;
    int M, N, K;
    int kmode;
    int lower_only;        // skip output tiles with tj > ti
    int tile_map;
    const GemmBatchItem* batch;  // nullable; grid.z = n_batch
    int n_batch;
    const int* info;       // nullable: if *info != 0 the kernel exits immediately
    hipStream_t stream;    // null: ctx->stream
    int nsplit;            // > 1: split-K over grid.y into split_buf (store epilogues only), then reduced
    double* split_buf; int64_t split_stride;
    int dma_ok;            // batched launches: 1 = every item meets gemm_dma_usable (checked by the caller)
    int skip_reduce;       // split-K: leave the slices in split_buf (the caller reduces them itself)
    int small64;           // 1: every M, N is a multiple of 64 and every K of 32: launches with few tiles may take gemm_small.hip
    // batched objective (filled in by the launchers from the context): grid.z = bz_div * bn, theta = blockIdx.z / bz_div,
    // A / B / C / info / split_buf of theta tb lie tb * bstride doubles behind those of theta 0
    int bn, bz_div;
    int64_t bstride;
};
// theta index and batch item of a GEMM workgroup
__device__ __forceinline__ void gemm_block_z(const GemmArgs& g, int z, int* tb, int* item) {
    if (g.bn > 1) { *tb = z / g.bz_div; *item = z - *tb * g.bz_div; }
    else { *tb = 0; *item = z; }
}
// The same for the launches of a batched evaluation (bn > 1), with the dispatch order taken apart again: workgroups start in
// the order of their linear index (x fastest, then z), and with the thetas in z the LONGEST tiles of the last theta -- the
// enumerations put long k-ranges first -- came behind all tiles of the thetas before it: a launch of K^-1 = V^T V for 16
// thetas at N = 4096 ended with a tail of up to 32 of its 187 slab units per workgroup slot.  Here the theta is the fastest
// index, then the batch item, then the tile: long tiles of ALL thetas first, the tail is made of the shortest ones; with a
// multiple of eight thetas all tiles of a theta also land on one XCD (round-robin dispatch) and share its L2.  Which
// workgroup computes a tile changes no bit.
// (With a multiple of eight thetas every theta sits on one XCD; any other count spreads them evenly.  Counting the thetas in
// eights -- surplus workgroups returning at once -- pins theta t to XCD t mod 8 for EVERY count, and was measured and dropped:
// two thetas then use two of the eight XCDs, nine load one XCD twice; a 42-restart fit at N = 4096, whose rounds run through
// all widths, went from 2.45 to 3.2 s.)
__device__ __forceinline__ bool gemm_block_order(const GemmArgs& g, int* bx, int* tb, int* item) {
    if (g.bn > 1) {
        const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.z;
        const int rest = lin / g.bn;
        *tb = lin - rest * g.bn;
        *bx = rest / g.bz_div;
        *item = rest - *bx * g.bz_div;
        return true;
    }
    *bx = (int)blockIdx.x; *tb = 0; *item = (int)blockIdx.z;
    return true;
}
static inline unsigned gemm_grid_z(const GemmArgs& g) { return (unsigned)(g.bz_div * g.bn); }
static inline void gemm_fill_batch(const gpry_ctx* ctx, GemmArgs* g) {
    g->bn = ctx->bn; g->bstride = ctx->bstride; g->bz_div = g->batch ? g->n_batch : 1;
}
// ---- stream-K launches of the DMA engine (gemm_dma.hip): the (tile, k) space of a launch is cut into segments of
// equal length, one workgroup per segment; a segment is a list of parts (tile, share of the tile's k-range).
struct GemmPart { int bz, ti, tj, lo, hi, slice; };     // lo / hi: slab pairs (32 k) within the tile's own k-range
struct GemmRedTile { int bz, ti, tj, nslice; };         // tiles whose product arrives in nslice >= 2 partial slices
struct GemmPartsPlan {
    GemmPart* d_parts = nullptr; int* d_first = nullptr; GemmRedTile* d_red = nullptr;
    int nwg = 0, nred = 0, max_slices = 0;
};
struct GemmShape { int M, N, K; };
// segment length (slab pairs) that gives `slots` segments over all tiles of the shapes
int gemm_parts_segment(int kmode, int lower_only, const std::vector<GemmShape>& shapes, int slots);
// plan for one launch (items = batch items in order; a non-batched launch has one); frees nothing on failure
int gemm_parts_plan_build(gpry_ctx* ctx, int kmode, int lower_only, const std::vector<GemmShape>& items, int seg_pairs,
                          GemmPartsPlan* out);
void gemm_parts_plan_free(GemmPartsPlan* pl);
int gemm_dma_parts_launch(gpry_ctx* ctx, const GemmArgs& g, bool a_trans, bool b_trans, int epi, const GemmPartsPlan& pl,
                          int64_t slice_stride);
// a_trans: A(i,k) stored at A[k*lda + i]; b_trans: B(k,j) stored at B[j*ldb + k]
int gemm_f64_launch(gpry_ctx* ctx, const GemmArgs& g, bool a_trans, bool b_trans, int epi);
// 64 x 64 tiles for launches with a handful of 128 x 128 tiles (gemm_small.hip); same bits
int gemm64_launch(gpry_ctx* ctx, const GemmArgs& g, bool a_trans, bool b_trans, int epi);
int gemm_split_scratch(gpry_ctx* ctx, int nsplit, int64_t slice, double** buf);
// gemm_dma.hip: LDS-DMA staged, software-pipelined variant for 128-aligned products (NN, NT, TN)
int launch_trtri_diag(gpry_ctx* ctx, const double* L, double* V, int64_t Np, hipStream_t st, bool zero_right = false);   // chol_panel.hip
// re-scales the training coordinates for the prediction factor if the last LML evaluation left its own in dXs
int ensure_pred_xs(gpry_ctx* ctx);   // kernel_build.hip
int launch_point_full(gpry_ctx* ctx, const double* x, int want_kinv, double* kstar, double* G, double* u, double* part,
                      double* mean_part, double* ss_part, double* out);
int launch_trtri_diag128(gpry_ctx* ctx, const double* L, double* V, int64_t Np, hipStream_t st, bool clear_right);   // trtri_small.hip
int launch_trtri_diag_range(gpry_ctx* ctx, const double* L, double* V, int64_t Np, int blk0, int nblk, hipStream_t st);
bool gemm_dma_usable(const GemmArgs& g, int M, int N, int K);
int gemm_dma_launch_product(gpry_ctx* ctx, const GemmArgs& g, bool a_trans, bool b_trans, int epi, dim3 grid);
int sweep_gemm_dma_sp_launch(gpry_ctx* ctx, const GemmArgs& g);  // sweep_gemm.hip: LDS-DMA staging + explicit software pipeline

// ---- kernel_build.hip --------------------------------------------------------------
int upload_params(gpry_ctx* ctx, const double* theta);
int launch_scale_train(gpry_ctx* ctx);                         // dXs from dX and theta
int launch_kernel_train(gpry_ctx* ctx, double* K, int add_noise, double* U = nullptr); // full symmetric K; U (nullable): the identity's tiles on and right of the diagonal (potrf_stacked)
int launch_kernel_rows(gpry_ctx* ctx, int64_t row0, int k, int64_t ldk, double* Bk, double* Cb);   // border rows of K
int launch_cross_build(gpry_ctx* ctx, const double* Xc, int64_t m0, int64_t mc,
                       int64_t ldk, double* Kst, double* mean_part, int raw_affine,
                       hipStream_t st = nullptr);
int launch_cross_prepare(gpry_ctx* ctx);               // centred scaled training rows for ...
int launch_cross_build_mfma(gpry_ctx* ctx, const double* Xc, int64_t m0, int64_t mc, int64_t ldk, double* Kst, double* mean_part,
                            int raw_affine, int hybrid = 0);           // ... the panel with MFMA distances (sweep, large predict batches); hybrid: near pairs from the coordinates
int launch_cross_mean_bound(gpry_ctx* ctx, const double* Xc, int64_t m0, int64_t mc, double* mean_part, double* sabs_part,
                            double ubnd, double uhi, unsigned long long* live_cnt);     // the bound pass of a pruned sweep
int launch_cross_build_small(gpry_ctx* ctx, const double* Xc, int64_t m0, int64_t mc, int64_t ldk,
                             double* Kst, double* mean_part, int raw_affine);     // 4 x (Np/128) mean partials
int launch_predict_mean_small(gpry_ctx* ctx, const double* Xc, int64_t M, int nsplit, double* part_out);
int launch_gates(gpry_ctx* ctx, const double* Xc, int64_t M, uint8_t* mask);
int launch_predict_small_std(gpry_ctx* ctx, const double* Xc, int M, double* kstar, double* mean_part,
                             double* ss_part);
int launch_gradx(gpry_ctx* ctx, const double* x, int raw_affine, int want_kinv, double* kstar, double* G,
                 double* u, double* w, double* part, double* out);
int launch_gradx_batch(gpry_ctx* ctx, const double* Xb, int64_t m, int raw_affine, const double* Wm, int64_t ldw,
                       double* out);
int launch_lml_small(gpry_ctx* ctx, int want_grad, double* out, int* info);   // lml_small.hip: N <= 128, d <= 16 in one launch, results picked up as they land; 1 = not applicable
int launch_lml_small_batch(gpry_ctx* ctx, int B, const double* params, int want_grad, double* out, int* info);   // out: B x (2 + 1 + GPRY_MAX_DIM)
int launch_lml_traces(gpry_ctx* ctx, const double* Kinv, const double* alpha,
                      double* grad_out_dev, const double* lq_dev, double* host_res, int info_at);
// host_res (nullable, mapped host memory): [logdet/2, quad, grad...] and dinfo[0..1] as doubles at info_at, status last

// ---- chol.hip ----------------------------------------------------------------------
int potrf_lower_fused(gpry_ctx* ctx, double* A, int64_t Np);       // panel steps, every trailing update its own launch (comparator)
int potrf_lower_overlap(gpry_ctx* ctx, double* A, int64_t Np);
int potrf_stacked(gpry_ctx* ctx, double* A, double* U, int64_t Np);      // A <- L, U <- L^-T (U: the identity on entry)
bool potrf_stacked_usable(const gpry_ctx* ctx, int64_t Np);
int transpose_upper_launch(gpry_ctx* ctx, const double* U, double* V, int64_t Np);     // panel step + earlier trailing tiles in ONE launch; above Np = 3584 segment by segment (default)
int trtri_lower(gpry_ctx* ctx, const double* L, double* V, double* T, int64_t Np);
// V = L^-1 queued phase by phase underneath potrf (chol.hip); begin returns 1 when the size is not cut
int trtri_pipeline_begin(gpry_ctx* ctx, const double* L, double* V, double* T, int64_t Np);
int trtri_pipeline_step(gpry_ctx* ctx, int blocks_done);
int trtri_pipeline_finish(gpry_ctx* ctx);
void trtri_pipeline_abort(gpry_ctx* ctx);   // error path: wait for the side stream, mark the chain inactive
void trtri_pipe_free(gpry_ctx* ctx);
int lauum_lower(gpry_ctx* ctx, const double* V, double* Kinv, int64_t Np);
int factor_chain_slices(gpry_ctx* ctx, int64_t Np, int* slices);   // split-K slices V = L^-1 and K^-1 = V^T V need at this size
int solve_alpha(gpry_ctx* ctx, const double* V, const double* y, double* z, double* alpha,
                int64_t Np);
int logdet_and_quad(gpry_ctx* ctx, const double* L, const double* z, int64_t Np,
                    double* out2_dev, double* host_res, int info_at);   // host_res: as above, value-only evaluation
int rocsolver_potrf_trtri(gpry_ctx* ctx, double* A, double* V, int64_t Np, int want_v);

// ---- server.hip: resident predict kernel --------------------------------------------
int require_model(gpry_ctx* ctx, bool need_factor);   // api.hip: training set, theta and (need_factor) factor present
int serve_stop(gpry_ctx* ctx);          // no-op when nothing is running; every model-changing entry point calls it first
void serve_free(gpry_ctx* ctx);
void serve_stats(gpry_ctx* ctx, int64_t* launches, int64_t* requests);
int serve_predict_mean(gpry_ctx* ctx, const double* X, int64_t M, double* part, int* nsplit_out, unsigned* gate_bits);
#define GPRY_SERVE_MAXM 8

// ---- api.hip: the factor chain of one objective evaluation, shared with loo_fit.hip ------
// A <- chol(K + diag(alpha)), V <- A^-1 at the theta the context holds (T: scratch); info_host NULL: the caller reads dinfo itself
int build_factor(gpry_ctx* ctx, double* A, double* V, double* T, int* info_host);
// the launches of one gpry_lml evaluation at the theta the context holds, shared with lml_hessian.hip: leaves L in dW, V in
// dW2, alpha at dvec + Np, [logdet/2, quad, grad ...] at dvec + 2 Np and, with want_grad, K^-1 (lower) in dW3; results and
// the status words (from LML_RES_INFO) go to `dres` (mapped host memory)
constexpr int LML_RES_INFO = 2 + GPRY_THETA_MAX;
int lml_chain(gpry_ctx* ctx, int want_grad, double* dres);
bool panel_timed_out(int marker);                       // fourth status word: a bounded wait of a panel step ran out
int panel_timeout_error(gpry_ctx* ctx, int marker);
// loo.hip: gpry_loo's pass over an inverse factor V (partial sums per 64 x 64 tile; ceil(N / 64) x Np doubles each)
int loo_pass_launch(gpry_ctx* ctx, const double* V, double* qpart, double* wpart);
// predict_thetas.hip: gpry_predict_thetas_var's cross-kernel panel (pt_var_panel_kernel) for the model the context holds, at
// its own theta: Kst[k * ldk + c], k < Np, c < cols (a multiple of 64 that covers npts); zeros from row N and column npts on
int pv_panel_launch(gpry_ctx* ctx, const double* dX, int64_t npts, int64_t cols, double* Kst, int64_t ldk);
// lml_hessian.hip: the d matrices dK / dlog l_k among the training rows (full zero-padded squares, Km + k Np^2) from the scaled
// rows the context holds, at its own theta: stage (b) of gpry_lml_hessian without its Hessian sums
int lml_hess_km_launch(gpry_ctx* ctx, double* Km);
// api.hip: the B thetas of a call in ONE chain of launches (arena of scratch sets, chunking, parameter and result staging) --
// the chain itself is the caller's: gpry_lml_batch's (lml_chain) or gpry_loo_objective_batch's (loo_fit.hip).  A chain is the
// code of a single evaluation that honours gpry_ctx::bn / bstride / bpar and writes theta tb's results to row tb of `dres`.
struct BatchChain {
    const char* name;                                       // stage timer and roctx range around a chunk; prefix of the messages
    int (*chain)(gpry_ctx* ctx, int want_grad, double* dres);
    bool latency_only;                                      // no throughput-schedule form: option "lml_schedule" is not read
    int64_t part_min, split_min;                            // doubles the chain's tail needs of the `part` and `split` pieces (0: the factor chain's)
    int head, info_at;                                      // result row: the gradient from `head`, the status words from `info_at`
    double (*value)(const double* row);                     // the objective from the row's head, without - N/2 log 2 pi
};
// returns 1 where fewer than two scratch sets fit (latency schedule: the caller evaluates one theta after another -- same bits)
int objective_batch_general(gpry_ctx* ctx, const BatchChain& bc, const double* thetas, int64_t B, int want_grad, double* value,
                            double* grad, int* info);

// ---- api.hip: the protocol of every entry point that evaluates a fit objective at thetas that are not the context's own
// (gpry_lml, gpry_lml_batch, gpry_loo_objective, gpry_loo_objective_batch, gpry_lml_hessian) ------
// Entry checks on B rows of ctx_ntheta entries: a training set is there, every entry is finite, d <= 32.  Stops the resident
// predict kernel, selects the device and disarms the adoption of gpry_lml's factor by gpry_factorize (gpry_ctx::lml_cache: an
// evaluation borrows the scratch that factor lives in; only gpry_lml arms it again, behind a chain that left a factor there).
int objective_entry(gpry_ctx* ctx, const char* name, const double* thetas, int64_t B);
// a chain's factor scaled the training coordinates for its own theta: they belong to the prediction factor, and whoever needs
// them next restores them (ensure_pred_xs).  `had`: the context held a theta of its own when the call came in.
static inline void note_xs_foreign(gpry_ctx* ctx, bool had) { if (had && ctx->factor_valid) ctx->xs_foreign = true; }
// installs `theta` as the context's for the length of a scope: the prediction factor (dA, dV, dalpha_) is not disturbed
struct ThetaScope {
    gpry_ctx* c; bool had; double saved[GPRY_THETA_MAX];
    ThetaScope(gpry_ctx* ctx, const double* theta) : c(ctx), had(ctx->have_theta) {
        memcpy(saved, ctx->theta, sizeof(saved));
        for (int k = 0; k < ctx_ntheta(ctx); k++) ctx->theta[k] = theta[k];
        ctx->have_theta = true;
    }
    ~ThetaScope() { memcpy(c->theta, saved, sizeof(saved)); c->have_theta = had; }
    void factor_chain_ran() { note_xs_foreign(c, had); }
};
// A result row [head ..., status words from info_at] in mapped host memory.  The last kernel of a chain writes the status
// words; until then they hold the "not written" marker.
static inline void objective_row_unwritten(double* row, int info_at) { row[info_at] = -1.0; row[info_at + 1] = -1.0; }
// the context's pinned staging buffer as the result row of a single evaluation (at least `bytes`), marked "not written"
int objective_row(gpry_ctx* ctx, int64_t bytes, int info_at, double** hres, double** dres);
// *info of evaluation `which` from its row, read behind a stream synchronisation; a row without status and a panel step whose
// bounded waits ran out are errors
int objective_status(gpry_ctx* ctx, const char* name, int64_t which, const double* row, int info_at, int* info);
// One stream synchronisation per single evaluation, also behind a chain that failed (rc != 0, which is returned): nothing of
// the call stays in flight.  Then objective_status of `row` (NULL: no chain ran, *info stays).
int objective_wait(gpry_ctx* ctx, const char* name, int rc, const double* row, int info_at, int* info);
// Value, gradient (grad != NULL: ctx_ntheta entries from g) and Hessian (hess != NULL: from h) of one evaluation as the caller
// gets them: `head` - N/2 log 2 pi, or with info != 0 the convention of sklearn:_gpr.py:586-589, -inf and zeros.
void objective_write(const gpry_ctx* ctx, int info, double head, const double* g, const double* h, double* value, double* grad,
                     double* hess);
// the head of gpry_lml's row [logdet/2, quad, grad ...]
static inline double lml_head(const double* row) { return -0.5 * row[1] - row[0]; }

// width class of the kernels that are instantiated per number of dimensions
static inline int dp_class(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 24 ? 24 : 32; }
// split-K count of an engine launch of `tiles` 128 x 128 output tiles over K = Np: only where the tiles leave most of the GPU
// idle and a slice keeps 256 of K
static inline int splitk_count(int64_t tiles, int64_t Np) {
    int nsplit = 1;
    while (nsplit < 4 && tiles * nsplit * 2 <= 1100 && Np / (nsplit * 2) >= 256) nsplit *= 2;
    return nsplit;
}

int ensure_capacity(gpry_ctx* ctx, int64_t N, int d);
int ensure_pinned(gpry_ctx* ctx, int64_t bytes);
