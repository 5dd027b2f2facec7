/*
 * gpry_hip.h -- C ABI of libgpry_hip.so: MI355X (gfx950) GP-regression + NORA sweep.
 *
 * This is the drop-in boundary for GPry's hot path.  GPry is pure Python; the calls
 * below are what a ctypes binding inside gpry/gpr.py and gpry/gp_acquisition.py would
 * bind to replace the numpy/scipy/scikit-learn arithmetic (reference file:line cited
 * per entry point; "sklearn:" = scikit-learn 1.7.2 sklearn/gaussian_process/).
 *
 * Conventions
 *  - plain C, no C++ types, no torch types; all host arrays are caller-owned,
 *    C-contiguous float64 / int64 / uint8; every call copies in/out synchronously and
 *    returns after the device work has completed (stream-synchronised).
 *  - return value: 0 ok; <0 API / HIP / RCCL error (text via gpry_last_error);
 *    numerical status (LAPACK-style "info") is returned through an out-parameter.
 *  - one gpry_ctx per device; a ctx is not re-entrant.
 *  - all floating point is IEEE float64.
 */
#ifndef GPRY_HIP_H
#define GPRY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpry_ctx gpry_ctx;
typedef struct gpry_comm gpry_comm;
typedef struct gpry_group gpry_group;

/* kernel ids: Product(ConstantKernel, RBF | Matern(nu)) -- gpry/kernels.py:213,281,601,681 */
enum { GPRY_RBF = 0, GPRY_MATERN12 = 1, GPRY_MATERN32 = 2, GPRY_MATERN52 = 3 };
/* Flag bit or-ed into a kernel id: Sum(Product(...), WhiteKernel(w)) -- gpry/kernels.py WhiteKernel / Sum.  The noise
 * level w (a variance, transformed-y units) is a hyperparameter of the model: the training matrix is
 * C k(X, X) + diag(alpha + w), the prior variance of a new point C + w, and while the flag is set EVERY theta / grad array
 * of gpry_set_theta, gpry_lml and gpry_lml_batch has 2 + d entries, the last being log w resp. d lml / d log w.
 * Without the flag nothing changes.  Entry points that do not carry the term yet refuse such a model with an error that
 * names the white term (-1, gpry_last_error) and leave the context as it was: gpry_maximize_acq, gpry_predict_cov,
 * gpry_sample_joint, gpry_group_*.  (The Kriging-believer session carries it: var0 = C + w - |u|^2, and the caller adds w
 * to the alpha of the points it appends.) */
#define GPRY_KERNEL_WHITE 0x10

/* Largest dimension of the parameter space: ABI size of the per-dimension arrays in gpry_affine AND the
 * limit gpry_set_train enforces (the kernels of this build are instantiated for d <= 32; GPry's design
 * envelope is d < 20, README.rst:64). */
#define GPRY_MAX_DIM 32

/* Affine pre-/post-processing fused into the device path.
 * x_ = (x - x_lo) / x_span       gpry/preprocessing.py:380 (Normalize_bounds.transform)
 * y  = y_ * y_std + y_mean       gpry/preprocessing.py:620 (Normalize_y.inverse_transform)
 * s  = s_ * y_std                gpry/preprocessing.py:630 (inverse_transform_scale)
 * y  = min(y, clip_hi)           gpry/gpr.py:1187-1195   (pass +inf for "no clipping") */
typedef struct {
    int has_x_affine;                 /* 0: X is used as given */
    double x_lo[GPRY_MAX_DIM];
    double x_span[GPRY_MAX_DIM];
    double y_mean, y_std;
    double clip_hi;
} gpry_affine;

/* One shortlisted candidate of the NORA sweep (gpry/gp_acquisition.py:1328-1333 feeds
 * candidates to RankedPool.add_one in descending acquisition order). */
typedef struct {
    double acq, y, sigma;
    int64_t idx;
} gpry_cand;

/* bit flags of the per-candidate mask consumed by predict/sweep */
enum {
    GPRY_MASK_CLASSIFIED_INF = 1, /* gpry/gpr.py:1145,1172,1230: mean=-inf, std=0      */
    GPRY_MASK_OUTSIDE_TRUST = 2   /* gpry/gpr.py:1107,1201:      mean=-inf, std kept   */
};

/* ---- library / device ------------------------------------------------------------ */
int gpry_version(void);
int gpry_device_count(int* n);
/* name (<=name_len), HBM bytes, CU count, max clock kHz, gcn arch string (<=arch_len) */
int gpry_device_info(int device, char* name, int name_len, int64_t* hbm_bytes,
                     int* n_cu, int* clock_khz, char* arch, int arch_len);

int gpry_ctx_create(int device, gpry_ctx** out);
int gpry_ctx_destroy(gpry_ctx* ctx);
const char* gpry_last_error(gpry_ctx* ctx); /* ctx may be NULL: last global error */
int gpry_ctx_sync(gpry_ctx* ctx);
/* Options (all of them; unknown keys and values outside the stated range return -1).  One comparator is kept per stage --
 * rocSOLVER for the factorisation ("chol"), the schedule with separate trailing launches for the fused Cholesky
 * ("chol_overlap"), the register-staged GEMM engine for the LDS-DMA one ("gemm_dma") --, the variants that lost their A/B
 * runs in earlier rounds are gone (profiles/HISTORY.md keeps their numbers).
 *   measurement
 *     "timing" 0/1            per-stage HIP-event timers (gpry_timing_get); off by default, switched on by gpry_timing_reset
 *   factorisation (gpry/gpr.py:1453-1465)
 *     "chol" 0/1              0 (default): hand-written MFMA Cholesky + V = L^-1; 1: rocSOLVER dpotrf / dtrtri (comparator)
 *     "chol_overlap" 0/1      1 (default): trailing-update tiles ride in the Cholesky panel launches (above 3584 padded rows
 *                             segment by segment: outer blocks of up to 768 columns, each followed by one SYRK launch, then
 *                             the last 3584 columns); 0: every update a launch of its own (comparator; bit-identical factors)
 *     "factor_pipeline" 0/1   V = L^-1 is queued phase by phase on a second stream underneath the Cholesky panel chain
 *                             (default 1; bit-identical), from "factor_pipeline_min" padded rows on (default 1280)
 *     "gemm_dma" 0/1          1 (default): LDS-DMA staged, software-pipelined GEMM engine for the sweep contraction and the
 *                             128-aligned products of the factor chain; 0: register-staged engine (comparator)
 *     "gemm_streamk"          largest padded size at which the top levels of V = L^-1 and K^-1 = V^T V run as stream-K
 *                             launches (default 5632; 0 = off)
 *     "gemm_small"            launches of at most this many 128 x 128 tiles use 64 x 64 tiles instead (default 32; 0 = never)
 *   objective (sklearn:_gpr.py:574-652)
 *     "lml_small" 0/1         gpry_lml of N <= 128, d <= 16 in ONE launch of one workgroup (default 1; the factor of such an
 *                             evaluation is not kept for gpry_factorize)
 *     "lml_cache" 0/1         gpry_factorize adopts the factor of the last gpry_lml when theta is the same (default 1)
 *     "lml_batch"             largest padded size at which gpry_lml_batch runs all its thetas through ONE chain of launches
 *                             (default 4096: beyond it the host's thread farm of three contexts is faster; 0 = one after another)
 *     "lml_batch_mb"          upper limit of the scratch arena of such a batch in MiB (default 49152; longer batches go in chunks)
 *                             (both also hold for gpry_loo_objective_batch, which shares the arena)
 *     "lml_schedule" 0/1      schedule of gpry_lml_batch above 128 rows.  0 (default) latency: every theta gets the launches -- and the
 *                             bits -- of a single gpry_lml.  1 throughput: the chain for many thetas at once (whole-tile products only,
 *                             the recursive inverse at every size, the Cholesky in column blocks with one SYRK launch behind each, the
 *                             thetas dealt over "lml_streams" streams); a theta's result does not depend on how many thetas share the
 *                             call (B = 1 included) and differs from the latency schedule's by rounding.  The host mirror sets it for
 *                             the multi-restart fits (gpry/gpr.py:968-984).  Concerns gpry_lml_batch alone: gpry_loo_objective_batch
 *                             always runs the latency schedule
 *     "lml_streams" 1..8      throughput schedule: stream groups per call (default 2)
 *     "tp_block", "tp_tail"   throughput schedule: width of the column blocks of the Cholesky (default 512) and size of the last
 *                             block, factored with riding tiles only (default 1024); multiples of 128.  No bit depends on them
 *     "tp_left" 0/1           throughput schedule: 0 (default) the column blocks right-looking (one launch of the block's width behind
 *                             every block), 1 left-looking (ONE deep launch in front of a block brings its columns up to date with
 *                             all columns left of it; the comparator, measured 1.5 % behind at 4096 rows).  Same factor bit for bit
 *     "chol_tp_segments" 0/1  1: every factorisation of the context takes those column blocks (comparator: the same factor bit for bit)
 *   predict / sweep (gpry/gpr.py:1022-1273, gpry/gp_acquisition.py:971-1108)
 *     "sweep_chunk"           candidates per sweep chunk, rounded up to a multiple of 1024 (default 0 = 32768 from 4096 padded
 *                             training rows on and proportionally more below: the K* panel of a chunk stays 1 GiB)
 *     "cross_mfma" 0/1        1 (default): the cross-kernel panel of sweeps and large predict batches takes its squared
 *                             distances from the matrix pipe (centred coordinates, |x|^2 + |y|^2 - 2 x.y); 0: the difference
 *                             form (comparator; gpry_kernel_cross, the small batches and Matern-1/2 always use it).  The form a sweep
 *                             actually took, and the error estimates of the model that decided it: gpry_sweep_info
 *     "cross_hybrid" 0/1      1 (default): a model whose error estimates rule the matrix-pipe form out because its length scales are
 *                             far below the extent of its data takes the hybrid form (matrix-pipe distances, every pair nearer than
 *                             r^2 = 100 again from the coordinates) instead of the difference form; 0: always the difference form
 *     "panel_debug"           test hooks, ORed bits: 32 the matrix-pipe panel whatever the estimates say, 64 every Cholesky panel step
 *                             reports a timed-out wait, 128 the scratch sets of a batched objective start as NaNs, 256 gpry_sweep_fetch
 *                             of a pruned sweep returns the arrays as they stand (bounds of y and acq where nothing was contracted)
 *                             without completing it (default 0)
 *     "topk_host"             largest pool that gpry_sweep_topk selects on the host from one kernel's records
 *                             (default 16384; 0 = always the device radix select)
 *     "predict_small"         mean-only gpry_predict of at most this many points is one fused launch (default 2048)
 *     "predict_split" 0/1     split-K contraction for gpry_predict batches of 5 ... a few thousand points (default 1)
 *     "sweep_upload" 0/1      gpry_sweep_logexp with a host pool: 1 (default) uploads it chunk by chunk on a copy stream, chunk
 *                             c + 1 underneath the kernels of chunk c (gpry/gp_acquisition.py:1023-1031 draws a fresh pool every
 *                             mc_every-th call); 0: one copy in front of the sweep (the comparator; same bits)
 *     "sweep_overlap" 0/1     1: the cross-kernel panel of chunk c + 1 is built on the side stream underneath the contraction of
 *                             chunk c (two panels; same bits).  Default 0: measured slower (profiles/r06_sweep.md), kept as the comparator
 *     "sweep_prune" 0/1       1: gpry_sweep_logexp with no arrays wanted builds only y and an exact upper bound of every candidate's
 *                             acquisition (its prior sigma); gpry_sweep_topk contracts only the candidates whose bound can reach
 *                             the shortlist (same records, bit for bit; see gpry_sweep_topk).  Default 0: the full sweep
 *     "sweep_mean_bound" 0/1  1 (default): such a sweep in the hybrid panel form (gpry_sweep_info) bounds y as well: its mean pass
 *                             skips every block of pairs too far apart to move y by more than ~1e-13 of the normalised targets,
 *                             adds a rigorous slack for them and for rounding, and computes y exactly only for the candidates it
 *                             contracts (same records and, after gpry_sweep_fetch, the same arrays bit for bit).  0: y exactly for
 *                             every candidate in the mean pass
 *     "sweep_screen" 0/1      1 (default): that mean pass certifies far blocks with an exact FP32 matrix product and a rigorous
 *                             margin in front of its FP64 test (gpry_sweep_screen_info); 0: the FP64 test alone (the comparator:
 *                             the same blocks are skipped, every array is the same bit for bit)
 *     "sweep_small_map" 0/1   1 (default): a one-pass contraction of at most 512 tiles of 128 x 128 (the compact batches of a pruned
 *                             sweep) launches one workgroup per tile, longest row tile first, consecutive candidate tiles on
 *                             different XCDs; 0: the super-tile map of the large launches (the comparator).  A row tile walks k in
 *                             the same direction under both maps: same bits
 *     "select_fused" 0/1      1 (default): the 12 passes of the device radix select of gpry_sweep_topk each derive the digit of the
 *                             pass before them from its own counters (no scan launches; per-wave aggregation of the histogram, one
 *                             atomic per workgroup in the emit); 0: a histogram and a scan launch per pass (the comparator; same set)
 *     "prune_one_select" 0/1  1 (default): the first contraction round of a pruned sweep answers from its own records when the Kp-th
 *                             exact value lies strictly above every bound outside them (no second select over the pool); 0: always
 *                             the select over all candidates (the comparator; same records and bound)
 *     "chol_stacked"          up to this padded training-set size (default 2048; at most 3584) the inverse factor V = L^-1 comes
 *                             out of the launches of the Cholesky factorisation itself (the identity appended to the matrix as
 *                             extra rows); 0: always the recursive inverse behind the factorisation.  Same L; V, and what is
 *                             computed from it, agree to rounding
 *     "chol_stacked_dense" 0/1  1: that schedule without use of the zero structure of the appended rows (every row block in
 *                             every step, every panel applied to every tile: three times the work; the comparator, same bits)
 *     "kb_rank" 0/1           1 (default): the Python mirror ranks an offer of the Kriging-believer pool through gpry_kb_rank
 *                             (one call: registration, batched Gram rows, the slot logic in C++); 0: its own loop over
 *                             gpry_kb_gram, one call per accepted point (the comparator; same picks, acq_cond to rounding)
 *     "svm_iters_per_launch"  gpry_svm_fit: updates one launch of its solver makes at most (default 4096; the result does
 *                             not depend on it)
 *     "predict_gates" 0/1     gpry_predict applies the gates of gpry_set_gates itself (default 0; the Python mirror sets 1)
 *     "predict_serve" 0/1     mean-only gpry_predict of <= 8 points is answered by a RESIDENT kernel (no launch per call;
 *                             default 1); "serve_idle_us" = how long that kernel waits for the next request before it
 *                             leaves (10 ... 1000000, default 2000)
 *     "mcmc_mapped" 0/1       gpry_mcmc_chains: 1 = the chains write their outputs straight to mapped pinned host memory; 0
 *                             (default) = to device memory, copied back once at the end of the call (same bits)
 * The environment variable GPRY_HIP_OPTIONS="key=value,key=value" applies options to every context the process
 * creates (gpry_ctx_create fails on an unknown key or a malformed entry). */
int gpry_ctx_set_option(gpry_ctx* ctx, const char* key, int64_t value);
/* current value of an option (the host mirror asks for "lml_batch" to decide whether the restarts of a fit -- gpry/gpr.py:968-984,
 * one after another there -- can be stepped side by side); unknown keys return -1 */
int gpry_ctx_get_option(gpry_ctx* ctx, const char* key, int64_t* value);

/* ---- model state ------------------------------------------------------------------ */
/* X_train_, y_train_, alpha = noise_^2 in the TRANSFORMED space, as assembled by
 * append_to_data (gpry/gpr.py:743-747).  X_ is N x d row-major.  The factor and any Kriging-believer session are dropped;
 * the resident candidate pool of gpry_sweep_logexp stays for a sweep with X == NULL under the new model unless d changes
 * (rows of another width are no pool of this model: such a sweep is refused). */
int gpry_set_train(gpry_ctx* ctx, const double* X_, const double* y_,
                   const double* alpha, int64_t N, int d);
/* kernel_.theta = [log C, log l_1..l_d] (sklearn:kernels.py:734-747); with kernel_id | GPRY_KERNEL_WHITE:
 * [log C, log l_1..l_d, log w], 2 + d entries */
int gpry_set_theta(gpry_ctx* ctx, int kernel_id, const double* theta);
int gpry_set_affine(gpry_ctx* ctx, const gpry_affine* tf);

/* ---- a1/a2/a8: kernel matrices ---------------------------------------------------- */
/* K = kernel_(X_train_) [+ diag(alpha)] -> host N x N.  gpry/gpr.py:1015-1016,
 * sklearn:kernels.py:931-966,1553-1560,1708-1738. */
int gpry_kernel_train(gpry_ctx* ctx, int add_alpha, double* K_out);
/* K* = kernel_(Xc_, X_train_) -> host M x N (gpry/gpr.py:1179).  Xc_ already
 * transformed; meant for tests and small M (the sweep never materialises it on host). */
int gpry_kernel_cross(gpry_ctx* ctx, const double* Xc_, int64_t M, double* K_out);

/* ---- a3/a7: factor (gpry/gpr.py:996-1020, 1453-1465) ------------------------------ */
/* builds K+diag(alpha), L = chol(K), V = L^-1, alpha_ = K^-1 y_.
 * *info = 0 ok, k>0: leading minor of order k is not positive definite (dpotrf). */
int gpry_factorize(gpry_ctx* ctx, int* info);
/* copy-out for attribute parity (L_, V_, alpha_); any pointer may be NULL */
int gpry_get_factor(gpry_ctx* ctx, double* L, double* V, double* alpha_);

/* ---- a15: grow the factor at fixed theta (bordered update instead of refactorising) ------------- */
/* append_to_data(X, y, fit_gpr=False, fit_classifier=False) (gpry/gpr.py:577-753): k more training
 * points with the hyper-parameters AND the pre-processors frozen, so that the old rows of X_train_,
 * y_train_ and alpha are unchanged.  The reference rebuilds K and refactorises (gpry/gpr.py:1015-1017,
 * O(N^3)); this extends L, V = L^-1 and alpha_ by border rows, O(k N^2) (two N x N x k products).
 * Xnew_: k x d, ynew_: k, alphanew: k (noise_^2), all in the TRANSFORMED space as in gpry_set_train.
 * *info = 0 ok; > 0: the enlarged matrix is not positive definite at that (1-based) column -- the
 * model is then left without a valid factor (re-send the training set and call gpry_factorize).
 * Used by the "lies" of BatchOptimizer (gpry/gp_acquisition.py:488-491) and RankedPool.cache_model
 * (:1550-1553). */
int gpry_append_rows(gpry_ctx* ctx, const double* Xnew_, const double* ynew_, const double* alphanew,
                     int64_t k, int* info);

/* ---- a4/a5: log marginal likelihood (+ gradient) ---------------------------------- */
/* sklearn:_gpr.py:574-652 via gpry/gpr.py:876-881.  Non-PD: returns 0 with
 * *lml = -inf, grad = 0, *info > 0 (sklearn:_gpr.py:586-589).  Does not disturb the
 * factor held for prediction.  grad has 1+d entries (ignored if want_grad == 0).  For a model set with GPRY_KERNEL_WHITE
 * theta and grad have 2+d entries: theta[1+d] = log w, grad[1+d] = 1/2 w (alpha^T alpha - tr K^-1); the other entries are,
 * to the bit, those of the model without the flag whose alpha is alpha + w.  A call that fails behind its first launch
 * returns after the stream has drained, as gpry_loo_objective and gpry_lml_hessian do: nothing of it stays in flight. */
int gpry_lml(gpry_ctx* ctx, const double* theta, int want_grad, double* lml,
             double* grad, int* info);

/* B evaluations of the same objective in one call (thetas: B x (1 + d), lml: B, grad: B x (1 + d) or NULL, info: B or NULL,
 * each as gpry_lml; rows of 2 + d entries, every theta with its own log w, for a model set with GPRY_KERNEL_WHITE).  The optimiser runs of a multi-restart fit (gpry/gpr.py:883-994, one after another there) stepped side
 * by side hand over one theta per run and round.  N <= 128, d <= 16: one launch, one workgroup per theta; larger training
 * sets up to option "lml_batch" padded rows (default 4096): ONE chain of launches in which every kernel (covariance build,
 * Cholesky panel steps, V = L^-1 levels, K^-1 = V^T V, traces) carries all thetas, each with its own scratch set; either way
 * every theta gets the arithmetic -- and the bits -- of a single gpry_lml call, and a theta whose matrix is not positive
 * definite returns (-inf, 0, info > 0) on its own.  Beyond that size the thetas are evaluated one after another. */
int gpry_lml_batch(gpry_ctx* ctx, const double* thetas, int64_t B, int want_grad, double* lml, double* grad, int* info);

/* ---- a8-a11: posterior mean / std (gpry/gpr.py:1022-1273, 1275-1352) -------------- */
/* X: M x d, raw if the affine map has_x_affine else already transformed.
 * mask (nullable): per-candidate GPRY_MASK_* bits.  mean/std in untransformed units,
 * clipped (clip_hi) and masked exactly as predict() does.  std may be NULL. */
int gpry_predict(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask,
                 double* mean, double* std);
/* Mean-only calls of <= 8 points -- the closures the nested samplers / MCMC call once per point
 * (gpry/gp_acquisition.py:766-771, 784-793; gpry/mc.py:387-391) -- do not launch a kernel: a resident kernel on
 * a stream of its own answers them through a mailbox in pinned host memory and leaves on its own when no request
 * arrives for "serve_idle_us".  Every other entry point stops it first (it holds the model of its launch), so the
 * caller sees nothing but the latency.  Same bits as the one-launch path ("predict_serve" = 0).
 * gpry_debug_serve_stats: launches of that kernel / requests it answered since the context was created. */
int gpry_debug_serve_stats(gpry_ctx* ctx, int64_t* launches, int64_t* requests);

/* ---- nested sampling of the posterior mean (nested.hip; bookkeeping in gpry_amd/nested.py) --------------------------
 * Replace the point-by-point likelihood calls of the reference's PolyChord / UltraNest runs (gpry/gp_acquisition.py:760-856:
 * `gpr.predict(np.atleast_2d(X), return_std=False, validate=False)[0]` per point).  The likelihood of a point is the
 * mean that gpry_predict returns for it alone, bit for bit: same slices and sums, y map, clip_hi, and the gates of
 * gpry_set_gates (-inf where they reject).  Draws: Philox4x32-10 keyed by `seed`, one fixed counter per draw, so the
 * results do not depend on scheduling.  lo / hi: d bounds of the prior box (lo < hi).  device_ms (nullable): device time
 * of the call.  Both need the factorised model.
 *
 * gpry_ns_prior: n points uniform on the box (point i, coordinates 2j and 2j + 1: counter (0, j, 0, i, 0)) and their
 *   y -- the live points of the reference's `nprior` start (gpry/gp_acquisition.py:814-817).  X_out: n x d, y_out: n. */
int gpry_ns_prior(gpry_ctx* ctx, const double* lo, const double* hi, uint64_t seed, int64_t n, double* X_out,
                  double* y_out, double* device_ms);
/* gpry_ns_generation: one generation of batch replacement -- k chains, chain c starting from a survivor drawn uniformly
 *   from X_surv (nsurv x d, their y y_surv), `num_repeats` slice-sampling steps on {x in the box : y(x) > lstar} along
 *   directions W z / |z| (W: d x d lower triangular in unit-cube coordinates, row-major -- a Cholesky factor; the
 *   contract is the triangle: row t is summed over columns 0 .. t, entries above the diagonal are never read).  A step
 *   steps out by whole widths, at most 32 per side, then makes up to 64 shrinkage tries; if all fail the chain keeps
 *   its point; a try outside the box costs no evaluation.  num_repeats = 0 returns the drawn starts.  Outputs the chains' last
 *   points X_new (k x d), their y (y_new) and the evaluations each chain made (ncalls, k).  Replaces one
 *   PolyChord iteration's `num_repeats` slice steps (gpry/gp_acquisition.py:650-682 settings, :760-813 run). */
int gpry_ns_generation(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv, const double* y_surv,
                       int64_t nsurv, double lstar, const double* W, uint64_t seed, int64_t generation, int k,
                       int num_repeats, double* X_new, double* y_new, int64_t* ncalls, double* device_ms);
/* gpry_ns_generation_clustered: gpry_ns_generation with one whitening matrix per cluster of the survivors.  W:
 *   n_clusters x d x d, row-major; labels: nsurv cluster numbers in 0 .. n_clusters - 1.  Chain c draws its starting
 *   survivor j as gpry_ns_generation does and walks with W + labels[j] d d; nothing else changes, so chain c equals, bit
 *   for bit, chain c of gpry_ns_generation called with that matrix.  (The clustering rule: gpry_amd/nested.py.) */
int gpry_ns_generation_clustered(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                                 const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                                 int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                                 double* X_new, double* y_new, int64_t* ncalls, double* device_ms);
/* gpry_ns_generation_volumes: gpry_ns_generation_clustered with the chains' clusters drawn in proportion to given
 *   probabilities (PolyChord's choice by prior volume).  cum_p: n_clusters non-decreasing cumulative probabilities, the
 *   last exactly 1.0.  Chain c draws its cluster q, the first q with u1 < cum_p[q] (u1: counter (1, 1, gen, c, 0), word
 *   a), then its start among q's survivors in their order in X_surv: index min(floor(u0 n_q), n_q - 1) with the u0 of
 *   gpry_ns_generation (counter (1, 0, gen, c, 0)), and walks with W + q d d; every step keeps its counter
 *   (gen, c, s).  Refused (-1) before anything runs: a label outside 0 .. n_clusters - 1, a decreasing (or negative,
 *   or NaN) cum_p, a last entry other than 1.0, a cluster with positive probability and no survivor.  Hence, bit for
 *   bit:
 *   - with one cluster and cum_p = {1.0}, the call equals gpry_ns_generation with that W;
 *   - a chain c that drew cluster q equals chain c of gpry_ns_generation called with q's survivors alone (in their
 *     order) and W + q d d: the same start from the same u0, the same step counters. */
int gpry_ns_generation_volumes(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                               const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                               int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                               const double* cum_p, double* X_new, double* y_new, int64_t* ncalls, double* device_ms);
/* gpry_ns_generation_phantoms: a generation that also keeps the chains' interior states (PolyChord's phantom points).
 *   The arguments of gpry_ns_generation_volumes with labels / cum_p nullable -- both NULL: the chains of
 *   gpry_ns_generation (n_clusters is then not read, W is d x d); labels alone: those of gpry_ns_generation_clustered;
 *   both: those of gpry_ns_generation_volumes -- and thin >= 1, X_ph, y_ph.  n_ph = (num_repeats - 1) / thin (0 for
 *   num_repeats = 0).  After step s (from 0) with (s + 1) % thin == 0 and s + 1 < num_repeats chain c's state and its y go
 *   to X_ph[(c n_ph + i) d ..] and y_ph[c n_ph + i], i = (s + 1) / thin - 1 (X_ph: k x n_ph x d, y_ph: k x n_ph,
 *   row-major); the last state is X_new as before and is not a phantom.  A chain whose step kept its point records that
 *   point again.  No draw, evaluation or counter is added or moved.  Hence, bit for bit:
 *   - X_new, y_new and ncalls equal those of the matching entry point above with the same arguments;
 *   - slot i of chain c equals X_new / y_new of chain c of that entry point called with num_repeats = (i + 1) thin;
 *   - every y_ph is gpry_predict of its row alone, and exceeds lstar unless the chain never moved.
 *   X_ph and y_ph both NULL: nothing is recorded (thin is still checked).  Refused (-1) before anything runs: thin < 1;
 *   exactly one of X_ph / y_ph NULL; X_ph and y_ph together above 2^30 bytes (8 k n_ph (d + 1)); and what the entry
 *   points above refuse.  The states are written to a device buffer of the context, which grows on demand, and copied
 *   out at the end; device_ms includes that copy. */
int gpry_ns_generation_phantoms(gpry_ctx* ctx, const double* lo, const double* hi, const double* X_surv,
                                const double* y_surv, int64_t nsurv, double lstar, const double* W, uint64_t seed,
                                int64_t generation, int k, int num_repeats, const int32_t* labels, int n_clusters,
                                const double* cum_p, double* X_new, double* y_new, int64_t* ncalls, int thin, double* X_ph,
                                double* y_ph, double* device_ms);
/* gpry_ns_knn: the k nearest other points of each of the n points X (n x d) in unit-cube coordinates
 *   u = (x - lo) / (hi - lo): nbr_out (n x k, row-major) holds row i's neighbours in order of (squared distance, index),
 *   i itself excluded, ties (duplicated points) broken by the index.  The squared distance is the sum over the
 *   coordinates, in their order, of the rounded squares (u_i - u_j)^2 -- a numpy restatement gives the same table.
 *   1 <= k <= 32, k + 1 <= n <= 65536; a non-finite u is refused.  Needs no model.  device_ms (nullable): device time of
 *   the call, copies included. */
int gpry_ns_knn(gpry_ctx* ctx, const double* lo, const double* hi, const double* X, int64_t n, int k, int32_t* nbr_out,
                double* device_ms);

/* ---- Metropolis MCMC of the posterior mean (mcmc.hip; adaptation, R - 1 and weights in gpry_amd/mcmc.py) ---------------
 * Replaces the point-by-point likelihood calls of the reference's Cobaya MCMC runs: the surrogate's final sample
 * (gpry/mc.py:173-327), GaussianKL's MC fallback at temperature 2 (gpry/convergence.py:430-476) and SmallChainProposer
 * (gpry/proposal.py:359-443).  The likelihood is that of the nested sampler above (gpry_predict of one point, bit for bit,
 * gates included).  gpry_mcmc_chains: `nchains` chains, one workgroup each, make `nsteps` Metropolis steps from the states
 * X0 (nchains x d) / y0 (nchains; NaN: the start is evaluated first and counted in ncalls).  Unit-cube coordinates
 * u = (x - lo) / (hi - lo); proposal u' = u + Lp z, Lp: d x d lower triangular, row-major, scale included; z ~ N(0, I) by
 * Box-Muller.  Step s of chain c draws from the counters (3, j, batch, c, s): j = 0..15 for z, 16 for the acceptance
 * uniform ua.  A proposal outside the box is rejected unevaluated; otherwise it is accepted iff its y' is finite,
 * y' > minus_inf_value and log(1 - ua) < (y' - y) / T.  Outputs: the state after every thin-th step (X_rec:
 * nchains x (nsteps / thin) x d, y_rec: nchains x (nsteps / thin); NULL allowed when nsteps < thin), the final states
 * X_last / y_last, per-chain accepted steps (naccept) and evaluations (ncalls).  X_prop / y_prop (both NULL, or
 * nchains x nsteps x d and nchains x nsteps): every proposal and its y, NaN where it was not evaluated -- a test hook,
 * no memory is set aside for it unless asked.  T > 0; d <= 32; lo < hi.  Stops the resident predict kernel first.
 * device_ms (nullable): device time of the call, copies included. */
int gpry_mcmc_chains(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                     int64_t nchains, const double* Lp, double T, double minus_inf_value, uint64_t seed, int64_t batch,
                     int nsteps, int thin, double* X_rec, double* y_rec, double* X_last, double* y_last,
                     int64_t* naccept, int64_t* ncalls, double* X_prop, double* y_prop, double* device_ms);
/* gpry_mcmc_ladders: tempered Metropolis ladders (parallel tempering; mcmc_ladders.hip, driven by gpry_amd/tempering.py),
 *   for surrogates with separated modes, which the chains above cannot leave.  `nladders` ladders of `nrungs` (1 .. 8)
 *   chains, one workgroup per ladder.  Slot r of ladder a is chain c = a nrungs + r; every per-chain array has the layout
 *   of gpry_mcmc_chains with nchains = nladders nrungs, in chain order c.  Slot r has its own proposal factor Lp[r]
 *   (Lp: nrungs x d x d) and temperature T[r]; its Metropolis step is that of gpry_mcmc_chains for chain c with Lp[r] and
 *   T[r]: the same counters (3, j, batch, c, s), box test and acceptance rule.  The proposals of a ladder's slots are
 *   evaluated together, in one pass over the training rows; each y is gpry_predict of its point alone, bit for bit.
 *   Swap rounds: if swap_every > 0 and (s + 1) % swap_every == 0, round q = (s + 1) / swap_every - 1 follows step s.  Its
 *   pairs are the slots (r, r + 1) with r = q (mod 2).  A pair is tried iff both current y are finite and above
 *   minus_inf_value; with us = the first uniform of the counters (3, 17, batch, c_r, s), c_r the chain of slot r, the swap
 *   is accepted iff log(1 - us) < (1 / T[r] - 1 / T[r + 1]) (y_{r+1} - y_r), and exchanges the states (x, u, y) of the two
 *   slots; temperatures and proposals stay with the slot.  The records of step s are taken after its swap round.
 *   Outputs: those of gpry_mcmc_chains, and nswap_try / nswap_acc (nladders x (nrungs - 1); NULL allowed when nrungs = 1):
 *   the swaps tried and accepted per ladder and adjacent pair.  Test hooks: X_prop / y_prop as in gpry_mcmc_chains;
 *   swap_log (nullable; nladders x (nsteps / swap_every) x (nrungs - 1)): 1 accepted, 0 tried and rejected, -1 not tried
 *   (the pairs of the other parity included).  With swap_every = 0 every output of slot r equals that of chain c of
 *   gpry_mcmc_chains called with Lp[r], T[r] and the same X0 / y0 / seed / batch, and nrungs = 1 is gpry_mcmc_chains; the
 *   outputs of ladder a do not depend on nladders or on the context.  Refused (-1, with gpry_last_error) before anything
 *   runs: nrungs outside 1 .. 8; a T[r] that is not positive and finite; swap_every < 0; nladders nrungs > 0x7fffffff;
 *   swap_log given with swap_every = 0; and what gpry_mcmc_chains refuses.  Staging as gpry_mcmc_chains ("mcmc_mapped"
 *   applies).  device_ms (nullable): device time of the call, copies included. */
int gpry_mcmc_ladders(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                      int64_t nladders, int nrungs, const double* Lp, const double* T, double minus_inf_value,
                      uint64_t seed, int64_t batch, int nsteps, int thin, int swap_every, double* X_rec, double* y_rec,
                      double* X_last, double* y_last, int64_t* naccept, int64_t* ncalls, int64_t* nswap_try,
                      int64_t* nswap_acc, double* X_prop, double* y_prop, int8_t* swap_log, double* device_ms);

/* ---- Hamiltonian Monte Carlo of the posterior mean (hmc.hip; adaptation, R - 1 and weights in gpry_amd/hmc.py) ----------
 * A second sampler for the same three uses as gpry_mcmc_chains (gpry/mc.py:173-327, gpry/convergence.py:430-476,
 * gpry/proposal.py:359-443), driven by the x-gradient of the mean, which is evaluated inside the kernel (one pass over
 * the training rows per gradient, as for the mean).  gpry_hmc_chains: `nchains` chains, one workgroup each, make `nsteps`
 * leapfrog trajectories from the states X0 (nchains x d) / y0 (nchains; NaN: the start is evaluated first and counted in
 * ncalls).  Unit-cube coordinates u = (x - lo) / (hi - lo), target exp(y / T).  Lp: d x d lower triangular, row-major, the
 * factor of the inverse mass matrix in unit-cube coordinates, no scale folded in.  Trajectory s of chain c draws from
 * the counters (4, j, batch, c, s): j = 0..15 for the momentum p = z ~ N(0, I) by Box-Muller, 16 for the acceptance
 * uniform ua, 17 for the step-size jitter u, eps_s = eps (0.8 + 0.4 u); a chain's bits do not depend on nchains.  The
 * trajectory: a half kick p += (eps_s / 2) Lp^T g(u) / T, then nleap times a drift u += eps_s Lp p followed by a kick (a
 * full one, the last a half one).  g is the gradient of the unclipped, ungated mean with respect to u: what
 * gpr.predict(x[None], return_mean_grad=True) returns (y_std included; that gradient is taken in the model's
 * transformed coordinates) times (hi - lo) / x_span, x_span the span of the model's x-affine map, 1 without one -- for a
 * model without an x-affine map the raw-coordinate gradient times (hi - lo).  A drift that leaves [0, 1]^d, or a gradient
 * that is not finite, rejects the trajectory at once and nothing further is evaluated; otherwise the end point's y' is
 * gpry_predict of it, bit for bit (clip and gates included), and the trajectory is accepted iff y' is finite,
 * y' > minus_inf_value and log(1 - ua) < (y' - y) / T - (|p'|^2 - |p|^2) / 2.  The gradient at the current state is kept
 * from one trajectory to the next inside a call, and evaluated once at the start of every call: two calls of k
 * trajectories with batch and batch + 1 draw other numbers than one call of 2 k, and count one gradient more.
 * Outputs: as gpry_mcmc_chains (X_rec, y_rec every thin-th trajectory, X_last, y_last, naccept, ncalls: evaluations of
 * the mean), and ngrad, the gradient evaluations per chain.  Test hooks, each nullable (X_prop and y_prop together), no
 * memory is set aside for one unless asked: X_prop (nchains x nsteps x d) / y_prop (nchains x nsteps), the last point of
 * every trajectory and its y, NaN where it was not evaluated; dH_prop (nchains x nsteps), the right-hand side of the
 * acceptance test, NaN likewise; G0 (nchains x d), g at the start states as the kernel computed it.  Refused (-1, with
 * gpry_last_error): d > 32; lo >= hi; T <= 0; eps <= 0; nleap outside 1 .. 1024.  Stops the resident predict kernel
 * first.  device_ms (nullable): device time of the call, copies included. */
int gpry_hmc_chains(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0, int64_t nchains,
                    const double* Lp, double eps, int nleap, double T, double minus_inf_value, uint64_t seed,
                    int64_t batch, int nsteps, int thin, double* X_rec, double* y_rec, double* X_last, double* y_last,
                    int64_t* naccept, int64_t* ncalls, int64_t* ngrad, double* X_prop, double* y_prop, double* dH_prop,
                    double* G0, double* device_ms);
/* gpry_hmc_chains_reflect: gpry_hmc_chains with an optional reflective drift (Neal 2011, section 5.5.1.5; with a mass
 *   matrix, specular reflection in the whitened coordinates q = Lp^-1 u).  reflect = 0: gpry_hmc_chains itself, bit for
 *   bit (max_reflect is not read; nreflect, if given, is set to 0).  reflect != 0: the drift of one leapfrog step is a
 *   billiard flow of duration tau = eps_s inside [0, 1]^d.  Repeat until the drift is done:
 *   1. velocity v_t = sum_{k <= t} rn(Lp[t][k] p_k), the sum of the plain drift in its order (rn: the product rounded to
 *      double before it is added; no FMA);
 *   2. hit times t_k = ((v_k > 0 ? 1.0 : 0.0) - u_k) / v_k where v_k != 0, +inf otherwise; j: the lowest index with the
 *      smallest t_k;
 *   3. no hit, or !(t_j < tau): u_t += rn(tau v_t), and the drift is done (a drift without a hit is the plain one, bit
 *      for bit);
 *   4. otherwise, if this drift has made max_reflect reflections already, the trajectory is rejected where it stands,
 *      unevaluated, as a box exit is by gpry_hmc_chains; else u_t += rn(t_j v_t) for t != j and u_j = the wall (1.0 for
 *      v_j > 0, else 0.0), p_k -= rn((rn(2 a) / b) r_k) for k <= j with r = row j of Lp, a = sum_{k <= j} rn(r_k p_k)
 *      (= v_j), b = sum_{k <= j} rn(r_k r_k), tau -= t_j, and the reflection is counted.
 *   After every move u is clamped to [0, 1], and after the drift x_t = lo_t + rn(u_t (hi_t - lo_t)) to [lo_t, hi_t]: both
 *   act at rounding level only.  Kicks, gradient, end point, acceptance rule, counters (no draw is added) and records are
 *   those of gpry_hmc_chains.  The chain stays exact: the flow is volume-preserving and time-reversible in q, a
 *   reflection keeps |p|^2, and the set of trajectories within the cap is invariant under "trajectory, then momentum
 *   flip".  nreflect (nullable, nchains): the reflections each chain made in this call.  Refused (-1) before anything
 *   runs: reflect != 0 with max_reflect outside 1 .. 1024, and what gpry_hmc_chains refuses. */
int gpry_hmc_chains_reflect(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                            int64_t nchains, const double* Lp, double eps, int nleap, double T, double minus_inf_value,
                            uint64_t seed, int64_t batch, int nsteps, int thin, double* X_rec, double* y_rec,
                            double* X_last, double* y_last, int64_t* naccept, int64_t* ncalls, int64_t* ngrad,
                            double* X_prop, double* y_prop, double* dH_prop, double* G0, int reflect, int max_reflect,
                            int64_t* nreflect, double* device_ms);

/* ---- Maximum and profiles of the posterior mean (maximize.hip; starts, H0, grids and continuation in
 * gpry_amd/maximize.py) ------------------------------------------------------------------------------------------------
 * gpry_maximize_mean: `nstart` local maximisations of the mean inside the box [lo, hi], one workgroup each, from the rows
 * of X0 (nstart x d) / y0 (nstart; NaN: the start is evaluated first and counted in ncalls).  No randomness.  Unit-cube
 * coordinates u = (x - lo) / (hi - lo).  The objective y(x) is gpry_predict of the point, bit for bit (clip and gates
 * included: a gated point is -inf).  The gradient g is that of the unclipped, ungated mean with respect to u, as in
 * gpry_hmc_chains.  fixed: d bytes, one mask per call; a coordinate with fixed[k] != 0 keeps the value X0 gives it, bit for
 * bit.  H0: d x d, row-major, symmetric positive definite, unit-cube coordinates: the first inverse-Hessian guess H and
 * the value H is reset to.  rn(.) below: the product rounded to double before it is added (no FMA); every sum runs in the
 * order of the coordinates, from 0.0.
 *   A start whose y is not finite or not > minus_inf_value, or which lies outside the box, ends at once with BAD_START
 *   (no gradient; G_out NaN); one whose first gradient is not finite with BAD_GRADIENT.  Then, from the state (u, y, g, H):
 *   1. Free set: k is free unless fixed[k], or u_k == 0 && g_k <= 0, or u_k == 1 && g_k >= 0.  No free coordinate, or
 *      max_{k free} |g_k| <= gtol: stop, CONVERGED_G.  Else, after max_iter iterations: stop, MAXITER.
 *   2. Direction: if the free set differs from the last iteration's and H != H0, H = H0 (a reset).  p_k = sum_{j free}
 *      rn(H_kj g_j) for free k, 0 otherwise.  If sum_{k free} rn(p_k g_k) is not > 0: with H != H0, H = H0 (a reset) and
 *      p again; with H == H0 stop, STALLED.
 *   3. Search: t = 1, 1/2, ..., at most max_halvings + 1 trials.  u'_k = clamp(u_k + rn(t p_k), 0, 1) for free k, u_k
 *      otherwise; x'_k = clamp(lo_k + rn(u'_k (hi_k - lo_k)), lo_k, hi_k) where u'_k != u_k (hi_k itself where u'_k == 1),
 *      x_k otherwise.  u' == u in
 *      every coordinate: stop, STALLED.  The trial is accepted iff y' = y(x') is finite, y' > minus_inf_value and
 *      y' >= y + rn(1e-4 sum_{k free} rn(g_k (u'_k - u_k))).  If every trial fails: with H != H0, H = H0 (a reset), p
 *      again and one more search; with H == H0 stop, STALLED (the normal end once improvements fall below the rounding
 *      of y).
 *   4. g' = the gradient at x'.  Not finite: the accepted point becomes the state, stop, BAD_GRADIENT.
 *   5. s = u' - u, q = g - g', both 0 outside the free set; sq = sum rn(s_k q_k), ss, qq likewise, Hq_k = sum_{j free}
 *      rn(H_kj q_j), qHq = sum rn(q_k Hq_k).  If sq > rn(1e-10 sqrt(rn(ss qq))): rho = 1 / sq, c = rn(rn(rho rho) qHq) + rho,
 *      H_kj = (H_kj - rn(rho (rn(s_k Hq_j) + rn(Hq_k s_j)))) + rn(c rn(s_k s_j)) for free k, j (H != H0 from here on).
 *   6. (u', y', g') becomes the state, the iteration is counted.  y' - y <= rn(ftol max(1, |y'|)): stop, CONVERGED_F.
 * Outputs per start: X_out (nstart x d), y_out, G_out (nstart x d; g at X_out), iters (completed iterations), ncalls
 * (evaluations of the mean), ngrad, status (0 CONVERGED_G, 1 CONVERGED_F, 2 STALLED, 3 MAXITER, 4 BAD_START,
 * 5 BAD_GRADIENT).  A start's outputs depend on its row alone, not on nstart, its position or the context.
 * Test hooks, all NULL or all given (no memory and no kernel code for them otherwise): U_tr (nstart x (max_iter + 1) x d),
 * y_tr (nstart x (max_iter + 1)), G_tr (as U_tr): the state at the start of iteration i, i = 0 .. iters; nhalv_tr and
 * reset_tr (nstart x max_iter, int): of every iteration that reached its search, the halvings of the accepted trial (-1:
 * none was accepted) and the resets of H.  Unused slots are NaN / -1.
 * Refused (-1, with gpry_last_error): d > 32; lo >= hi; max_iter outside 0 .. 100000; max_halvings outside 0 .. 1000; gtol or
 * ftol negative or not finite; an H0 entry that is not finite.  Stops the resident predict kernel first.  device_ms
 * (nullable): device time of the call, copies included. */
int gpry_maximize_mean(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, const double* y0,
                       int64_t nstart, const unsigned char* fixed, const double* H0, int max_iter, int max_halvings,
                       double gtol, double ftol, double minus_inf_value, double* X_out, double* y_out, double* G_out,
                       int* iters, int64_t* ncalls, int64_t* ngrad, int* status, double* U_tr, double* y_tr, double* G_tr,
                       int* nhalv_tr, int* reset_tr, double* device_ms);

/* ---- Maximum of the LogExp acquisition (maximize_acq.hip; starts and H0 in gpry_amd/maximize.py: maximize_acq, and
 * gpry_amd/gp_acquisition.py: BatchOptimizer(acq_optimizer="device")) ---------------------------------------------------
 * gpry_maximize_acq: `nstart` local maximisations of a(x) = 2 zeta (y(x) - baseline) + log sqrt(sigma(x)^2 - sigma_n^2)
 * inside the box [lo, hi], one workgroup each, from the rows of X0 (nstart x d).  The statement of the algorithm is that of
 * gpry_maximize_mean, word for word -- free set, direction, Armijo search, the stops, the resets of H, the BFGS update, the
 * rn(.) fences, the status codes, the layout of the traces -- with these differences:
 *   - the objective is a(x) instead of y(x), and the gradient g is the exact gradient of a with respect to u;
 *   - a start is always evaluated first (there is no y0 argument) and counted in ncalls.
 * Objective, per point x (raw coordinates): y = gpry_predict of the point, bit for bit, clip and gates included.
 * k*_j = C kappa(|x / l - X_j / l|), j < N.  u = V k* with V = L^-1 (row i over the columns 0 .. i; rows and columns >= N
 * are not read), ss = sum u_i^2, both in a fixed order.  sigma = sqrt(max(C - ss, 0)) y_std, and 0 where the classifier of
 * the device gates rejects the point.  a = LogExp.f(y, sigma) exactly as the sweep computes it (the same device function:
 * rn(sigma sigma) - rn(sigma_n sigma_n), clamped at 0, log sqrt, + rn((2 zeta) (y - baseline))).  a counts as -inf unless
 * y is finite, y > minus_inf_value and dv = rn(sigma sigma) - rn(sigma_n sigma_n) > 0 (the reference's mask,
 * gpry/acquisition_functions.py:983-992): such a trial is never accepted, such a start ends with BAD_START (a_out -inf).
 * Gradient, at a start and at an accepted trial: w = V^T u (= K^-1 k*), in a fixed order; with G_jk = d k(x, X_j) / d x_k
 * in the kernel's coordinates (gpry_predict_grad), m = G^T alpha_ and v = G^T w (d sigma_^2 / dx = -2 v in transformed
 * units), and s_k = (hi_k - lo_k) / x_span_k (x_span_k = 1 without an x-affine map):
 *   g_k = s_k (rn(rn((2 zeta) y_std) m_k) + rn(rn(y_std y_std) (-v_k)) / dv).
 * This is the gradient of the value the search tests, d/du [2 zeta y + (1/2) log(sigma^2 - sigma_n^2)].  It is NOT the
 * reference's BaseLogExp gradient std_grad / (std - sigma_n) + 2 zeta mu_grad (gpry/acquisition_functions.py:993-1007),
 * which is the derivative of log(sigma - sigma_n): its sigma term differs from the one above by the factor
 * (sigma + sigma_n) / sigma (and carries y_std once more, gpry/gpr.py:1236-1266); an Armijo search needs the gradient of
 * its own value.  A gradient with a component that is not finite: BAD_GRADIENT, as in gpry_maximize_mean.
 * Outputs per start: X_out (nstart x d), a_out, y_out and sigma_out (of X_out), G_out (nstart x d; g at X_out, NaN after
 * BAD_START), iters, ncalls (evaluations of a: passes over V), ngrad (gradients: second passes over V), status.  A start's
 * outputs depend on its row alone, not on nstart, its position or the context.  Test hooks as in gpry_maximize_mean, a_tr
 * in the place of y_tr.
 * Refused (-1, with gpry_last_error) before anything runs: what gpry_maximize_mean refuses; sigma_n negative or not finite;
 * zeta or baseline not finite; a model of more than 4096 padded rows (the kernel keeps k*, u and w of a point in LDS).
 * Stops the resident predict kernel first.  device_ms (nullable): device time of the call, copies included. */
int gpry_maximize_acq(gpry_ctx* ctx, const double* lo, const double* hi, const double* X0, int64_t nstart,
                      const unsigned char* fixed, const double* H0, double zeta, double baseline, double sigma_n,
                      int max_iter, int max_halvings, double gtol, double ftol, double minus_inf_value, double* X_out,
                      double* a_out, double* y_out, double* sigma_out, double* G_out, int* iters, int64_t* ncalls,
                      int64_t* ngrad, int* status, double* U_tr, double* a_tr, double* G_tr, int* nhalv_tr, int* reset_tr,
                      double* device_ms);

/* ---- Value, gradient and Hessian of the posterior mean at a batch of points (hessian.hip; the Gaussian approximation,
 * the Laplace evidence and covmat="laplace" in gpry_amd/maximize.py: hessian_gp, laplace_gp) ------------------------------
 * The reference stops at first derivatives (gpry/gpr.py:1236-1266 with gpry/kernels.py:257-278 RBF, :326-432 Matern).
 * gpry_hessian_mean: X (npts x d, raw coordinates), one workgroup per point, one launch.  Outputs in raw coordinates and
 * units of y:
 *   y_out (npts)          gpry_predict of the point, bit for bit, clip and gates included (a gated point is -inf);
 *   g_out (npts x d)      the gradient of the unclipped, ungated mean: gpry_predict_grad's mean_grad times
 *                         y_std / x_span_k (x_span_k = 1 without an x-affine map);
 *   H_out (npts x d x d)  the Hessian of the same mean, row-major, symmetric to the last bit (the lower triangle is
 *                         computed, the upper one copied); finite for a gated point too.
 * With diff_j = x / l - X_j / l, r = |diff_j|, w(r) the radial factor of the gradient (-exp(-r^2/2) RBF, -3 exp(-sqrt3 r)
 * Matern 3/2, -(5/3) (1 + sqrt5 r) exp(-sqrt5 r) Matern 5/2) and q(r) = w'(r) / r (exp(-r^2/2); 3 sqrt3 exp(-sqrt3 r) / r,
 * 0 at r = 0; (25/3) exp(-sqrt5 r)):  S_ab = sum_j alpha_j q_j diff_ja diff_jb,  T = sum_j alpha_j w_j,
 *   H_ab = y_std C (S_ab + T delta_ab) / (l_a l_b x_span_a x_span_b).
 * The bits of y, g and H depend on the model and the point alone, not on npts, the point's position or the context.
 * Refused (-1, with gpry_last_error) before anything runs: a NULL pointer; npts < 1 or > 2^31 - 1; no model; d > 32; a
 * Matern-1/2 model (its mean is not differentiable at the training rows); a coordinate that is not finite.  Stops the
 * resident predict kernel first.  device_ms (nullable): device time of the call, copies included. */
int gpry_hessian_mean(gpry_ctx* ctx, const double* X, int64_t npts, double* y_out, double* g_out, double* H_out,
                      double* device_ms);

/* ---- Joint posterior covariance and joint draws of the surrogate at a batch of points (joint.hip; the spread of the
 * posterior mean, covariance and evidence over realisations of the surrogate in gpry_amd/mc.py: surrogate_spread) ------
 * The reference returns no covariance (gpry/gpr.py:1062-1067); the closed form is sklearn's (_gpr.py:430-438).
 * gpry_predict_cov: X (m x d, raw coordinates as in gpry_predict), 1 <= m <= 4096.  With U = V K*^T (V = L^-1):
 *   cov (m x m, row-major)  y_std^2 (K(X*, X*) - U^T U), in units of y^2.  The lower triangle is computed and the upper
 *                           one copied: cov == cov^T to the last bit.  The diagonal is NOT clamped at 0 (gpry_predict's
 *                           std is sqrt(max(0, .)) of it).  A row with GPRY_MASK_CLASSIFIED_INF (the caller's mask, with
 *                           the device gates ORed in under option "predict_gates") has a zero row and column
 *                           (gpry/gpr.py:1145); GPRY_MASK_OUTSIDE_TRUST changes the mean only.
 *   mean (nullable, m)      finalised as gpry_predict does: y map, clip_hi, -inf where the merged mask has a bit.  The
 *                           sum over the training rows is the cross-kernel panel's (as in gpry_predict_grad_batch).
 * The k-ranges of the two products are split by the model size alone: cov[a][b] depends on the model and the two points,
 * not on m, on the points' positions in the batch or on the context.
 * gpry_sample_joint: S joint draws (1 <= S <= 65536) at the same kind of batch, Y (S x m, units of y):
 *   Y_s = mu + L_c z_s,  mu the UNCLIPPED, UNGATED mean (the clip belongs to the mean, not to a realisation of f; `mean`,
 *   nullable, is still the finalised mean of gpry_predict_cov), L_c the lower Cholesky factor of cov + eps C y_std^2 I.
 *   A classifier-rejected row is -inf in every draw and takes no part (identity on its diagonal in the factored matrix).
 *   eps starts at `jitter` (>= 0; a negative argument means 1e-10).  When the factorisation meets a pivot that is not
 *   positive -- or a pivot l^2 <= 8 (m + 1) 2^-53 max diag, i.e. zero within the factorisation's own backward error -- eps
 *   goes to 1e-14 (from 0) or to 100 eps and the matrix is factored again; above 1e-4 the call fails with -3, `info` the
 *   1-based pivot.  jitter_used: the eps of the factor that was used (the ladder is deterministic).
 *   z_s,j: Box-Muller (cos for even j, sin for odd j) of the two uniforms of Philox4x32-10 with counter
 *   (5 << 24, s, j / 2, 0) and key `seed`: a function of (seed, s, j) alone.  Y_s,i sums j ascending in a fixed tiling:
 *   draw s has the same bits whatever S.
 *   Z_out (nullable, S x m) the variates, Lc_out (nullable, m x m) the factor with a zero upper triangle.
 * Both refuse (-1, with gpry_last_error) before anything runs: a NULL required pointer (X, cov, Y); m or S out of range;
 * no factorised model; d > 32; a coordinate that is not finite; a jitter that is NaN or infinite.  Both stop the resident
 * predict kernel first.  device_ms (nullable): device time of the call, copies included. */
int gpry_predict_cov(gpry_ctx* ctx, const double* X, int64_t m, const uint8_t* mask, double* mean, double* cov,
                     double* device_ms);
int gpry_sample_joint(gpry_ctx* ctx, const double* X, int64_t m, const uint8_t* mask, int64_t S, unsigned long long seed,
                      double jitter, double* mean, double* Y, double* Z_out, double* Lc_out, int* info,
                      double* jitter_used, double* device_ms);

/* ---- Cross-validation of the training set from the resident factor (loo.hip; the report in gpry_amd/mc.py: validate_gp) --
 * Rasmussen & Williams section 5.4.2, at the current theta and with the y map as it is (nothing is refitted).  With
 * V = L^-1, K^-1 = V^T V, alpha_ = K^-1 y_ and the noise vector `alpha` of gpry_set_train (sigma_n^2, transformed units):
 * gpry_loo: N doubles each, any pointer may be NULL, all in units of y (y^2):
 *   mean, var_y   the predictive of the OBSERVATION y_i from all other points: y_i - alpha_i / q_i and 1 / q_i with
 *                 q_i = (K^-1)_ii = sum_k V_ki^2;
 *   var_f         max(1 / q_i - sigma_n,i^2, 0): the latent variance, what gpry_predict's std^2 of the model without
 *                 point i is at x_i;
 *   seq_mean, seq_var_y   the predictive of y_k from the points BEFORE it (one-step-ahead): y_k - w_k / V_kk and
 *                 1 / V_kk^2 with w = V y_; its z-score is w_k, and the log densities sum to the log marginal likelihood.
 *   One pass over the lower triangle of V in 64 x 64 tiles, the partial sums added in ascending tile order: q_i and w_k
 *   depend bit for bit on the model alone (not on the context, nor on which outputs are asked for: both are always formed).
 * gpry_leave_out: `ngroups` index sets, group g = idx[offsets[g] .. offsets[g + 1]) (offsets[0] = 0), each of 1 to 64
 *   distinct indices in [0, N); groups may overlap.  With B = (K^-1)_GG = V[:, G]^T V[:, G] (FP64 matrix pipe, the rows
 *   split by the model size alone) and delta = B^-1 alpha_G:
 *   mean (one per index, in the order of idx)          y_G - delta, the joint predictive mean of y_G from the rest;
 *   cov (the n_g x n_g blocks one after another)       B^-1 y_std^2, rows and columns in the order of idx;
 *   chi2 (ngroups)     alpha_G^T delta = (y_G - mean)^T cov^-1 (y_G - mean), n_g degrees of freedom;
 *   logpdf (ngroups)   log N(y_G; mean, cov), the density in units of y: -chi2 / 2 + log det B / 2 - n_g (log(2 pi) / 2 + log y_std);
 *   info (ngroups)     0, or the 1-based pivot (indices ascending) at which B was not positive definite: that group's
 *                      outputs are NaN, the call and the other groups are not affected.
 *   Every group's indices are sorted on the host and its outputs handed back in the caller's order: a group's results
 *   are the same bits whatever the order of its indices (up to that permutation), whatever other groups share the call
 *   and wherever it stands in the list.  All output pointers may be NULL.
 * Both refuse (-1, with gpry_last_error) when the context holds no valid factor; gpry_leave_out also an empty group, one
 * of more than 64 points, an index outside [0, N) and an index twice in a group.  Both work on the factor grown by
 * gpry_append_rows, stop the resident predict kernel first, and read V, alpha_, y_ and the noise vector only: the state of
 * gpry_predict, of a sweep, of a Kriging-believer session and of the samplers is untouched.  Stage timers "loo" and
 * "leave_out" (gpry_timing_get).  device_ms (nullable): device time of the call, copies included. */
int gpry_loo(gpry_ctx* ctx, double* mean, double* var_y, double* var_f, double* seq_mean, double* seq_var_y,
             double* device_ms);

/* ---- The leave-one-out log predictive density as a fit objective (loo_fit.hip; gpry_amd/gpr.py: loo_log_predictive,
 * fit_gpr_hyperparameters(objective="loo")).  Rasmussen & Williams section 5.4.2, in transformed units like the LML:
 *   L(theta) = sum_i [ 1/2 log q_i - alpha_i^2 / (2 q_i) ] - N/2 log 2 pi,   q_i = (K^-1)_ii, alpha = K^-1 y_
 * i.e. the sum of gpry_loo's Gaussian log densities of y_i under (mean, var_y), plus N log y_std.  The gradient is ONE set
 * of traces: with c_i = -1/2 (1 + alpha_i^2 / q_i) / q_i, b = K^-1 (alpha / q) and H = diag(sqrt(-c)) K^-1,
 *   dL / d theta_j = sum_kl [ 1/2 (b alpha^T + alpha b^T) - H^T H ]_kl (dK / d theta_j)_kl       for every j at once:
 * on top of gpry_lml with gradient one lower-only N^3 product on the matrix pipe, one matrix-vector product and
 * gpry_loo's pass over V (q has the bits gpry_loo gives for the same model).
 * theta / grad as gpry_lml (1 + d entries, 2 + d with GPRY_KERNEL_WHITE).  Non-PD: returns 0 with *value = -inf, grad = 0,
 * *info > 0.  Does not disturb the factor held for prediction, a Kriging-believer session, the resident pool or the
 * buffers of gpry_loo; it clears the factor cache of gpry_lml (option "lml_cache"), whose scratch it overwrites.  The
 * entry checks are gpry_lml's (training set present, theta finite, d <= 32; the resident predict kernel is stopped).  Any
 * size goes through the general chain (N <= 128 at 128 padded rows); one evaluation per call.  A result's bits depend on
 * (training set, theta, kernel id) alone, and the value's not on want_grad.  Stage timers: those of the factor chain,
 * "solve_alpha", "loo_q", "lauum", "loo_mirror", "loo_gram", "loo_traces". */
int gpry_loo_objective(gpry_ctx* ctx, const double* theta, int want_grad, double* value, double* grad, int* info);
/* B evaluations of gpry_loo_objective in one call: the optimiser runs of a multi-restart "loo" fit stepped side by side
 * (gpry/gpr.py:968-984 runs the restarts one after another; gpry_amd/lockstep.py), the twin of gpry_lml_batch and with its
 * arguments: thetas is B rows of 1 + d (2 + d with GPRY_KERNEL_WHITE) entries, value B, grad B rows, info (nullable) B.
 * From 128 padded rows up to option "lml_batch": ONE chain of launches for the thetas of a chunk (grid.z; at most 96, and
 * what option "lml_batch_mb" and 70 % of the free device memory hold of scratch sets), always in the latency schedule --
 * option "lml_schedule" concerns gpry_lml_batch alone.  Above "lml_batch", with "chol" != 0 or where fewer than two scratch
 * sets fit: one gpry_loo_objective after another.  Per theta, value, gradient and info are bit for bit those of
 * gpry_loo_objective on the same model, whatever B, the position in the batch, the chunking and the neighbours; a theta
 * whose matrix is not positive definite gives -inf, a zero gradient row and info > 0 and leaves the other rows alone.
 * Refused with an error: NULL pointers, B <= 0, a theta entry that is not finite.  State contract: gpry_loo_objective's.
 * Stage timer "loo_batch" around a chunk, beside the per-stage ones. */
int gpry_loo_objective_batch(gpry_ctx* ctx, const double* thetas, int64_t B, int want_grad, double* value, double* grad,
                             int* info);
int gpry_leave_out(gpry_ctx* ctx, const int64_t* idx, const int64_t* offsets, int64_t ngroups, double* mean, double* cov,
                   double* chi2, double* logpdf, int* info, double* device_ms);

/* ---- The Hessian of the log marginal likelihood in theta (lml_hessian.hip; gpry_amd/gpr.py: lml_hessian,
 * gpry_amd/hyper.py: hyper_laplace).  theta = [log C, log l_1 .. log l_d], log w last with GPRY_KERNEL_WHITE, p entries;
 * K = C k(r^2) + diag(alpha + w), r^2 = sum_k D_k, D_k(a,b) = ((x_ak - x_bk) / l_k)^2, alpha_ = K^-1 y_,
 * W = alpha_ alpha_^T - K^-1, K_i = dK / dtheta_i, K_ij = d2K / dtheta_i dtheta_j, transformed units like gpry_lml:
 *   H_ij = 1/2 tr(W K_ij) - (K_i alpha_)^T K^-1 (K_j alpha_) + 1/2 tr(K^-1 K_i K^-1 K_j)
 *   K_0 = C k (no noise on the diagonal), K_i = C h D_i (d k / d log l_i = h D_i), K_w = w I;
 *   K_00 = K_0, K_0i = K_i, K_ww = w I; EVERY cross entry with log w is zero, (log C, log w) included;
 *   K_ij = C (g D_i D_j - 2 delta_ij h D_i) for two length scales, g = -2 dh / dr^2: RBF g = k; Matern-1/2
 *   g = e^-r (1 + r) / r^3; Matern-3/2 g = 9 e^-t / t, t = sqrt(3) r; Matern-5/2 g = 25/3 e^-t, t = sqrt(5) r.
 * At r = 0 (the diagonal, duplicated rows) D_i D_j = 0: the second-derivative entry is defined as 0 there for every
 * kernel, as h is for Matern-1/2.
 * lml, grad (p): bit for bit gpry_lml(theta, want_grad = 1) on the same context.  hess: p x p row-major, symmetric to the
 * last bit.  (Where gpry_lml answers from its single launch -- N <= 128, d <= 16, option "lml_small" -- lml and grad come
 * from that launch and hess from the chain at 128 padded rows, whose own gradient agrees with it to rounding: there
 * "row 0 of hess is grad" holds to rounding, not to the bit.)  Not positive definite: returns 0 with *lml = -inf, grad and hess all zero, *info > 0 (gpry_lml's
 * convention); a panel time-out is an error.  Refused with -1 and a message: NULL arguments (device_ms may be NULL), a
 * theta entry that is not finite, no training set, d > 32, and a model of more than 4096 padded rows (the limit of
 * gpry_predict_cov and gpry_maximize_acq; refused before anything is launched, the context answers the next call as
 * before).  Cost: the d products K^-1 K_i, 2 N^3 each, in one batched launch of the GEMM engine, and O(p^2 N^2) besides;
 * scratch of its own: (1 + 2 d) Np^2 doubles (8.7 GB at 4096 rows, d = 32), allocated on first use, released with the
 * context, given back when gpry_set_train brings a model of less than half that footprint.  Models below 128 rows take
 * the chain at 128 padded rows.
 * State contract: evaluates at the theta passed in; the context's theta, the factor held for prediction, a
 * Kriging-believer session, the resident pool and the buffers of gpry_loo are not touched; the factor cache of gpry_lml
 * (option "lml_cache") is cleared, whose scratch it overwrites.  A result's bits depend on (training set, theta, kernel
 * id) alone: not on earlier calls, not on which context of a device evaluates it.  Stage timers: those of gpry_lml with
 * gradient, then "hess_pairs", "hess_products", "hess_btraces", "hess_middle", "hess_finish".  device_ms (nullable):
 * device time of the call. */
int gpry_lml_hessian(gpry_ctx* ctx, const double* theta, double* lml, double* grad, double* hess, int* info,
                     double* device_ms);

/* ---- The derivative of the posterior mean in theta at a batch of points (theta_grad.hip; gpry_amd/gpr.py:
 * mean_theta_grad, gpry_amd/hyper.py: hyper_spread).  theta = [log C, log l_1 .. log l_d], log w last with
 * GPRY_KERNEL_WHITE, p entries, at the theta of the factor the context holds; K = C phi(r) + diag(alpha + w),
 * alpha_ = K^-1 y_.  With diff_ia = x_a / l_a - X_ia / l_a, r_i = |diff_i|, k_i = C phi(r_i) and h(r) = -phi'(r) / r (minus
 * the radial factor of the x-gradient: exp(-r^2/2) RBF, exp(-r) / r Matern 1/2, 3 exp(-sqrt3 r) Matern 3/2,
 * (5/3) (1 + sqrt5 r) exp(-sqrt5 r) Matern 5/2), so that d k_i / d log l_a = C h(r_i) diff_ia^2 (Matern 1/2: 0 at r = 0, the
 * limit of h diff^2):
 *   U_0 = (alpha + w) o alpha_,   U_a = (dK / dlog l_a) alpha_,   U_w = w alpha_,   W = K^-1 U = V^T (V U)   (N x p)
 *   G_0(x) = y_std sum_i k_i W_i0,   G_a(x) = y_std sum_i (C alpha_i h(r_i) diff_ia^2 - k_i W_ia),   G_w(x) = -y_std sum_i k_i W_iw.
 * The log C entry is formed as k*^T K^-1 (D alpha_) as written, never as a difference of two O(1) numbers.  No
 * factorisation: W costs one N x N pass over the training rows and two triangular products with p right-hand sides, every
 * point after that one pass over the training rows.  A Matern-1/2 model is served: the derivative in theta exists at the
 * training rows too.
 * X (npts x d, raw coordinates where the affine map has an x-affine, as for gpry_hessian_mean); npts is unbounded (chunks of
 * 65536 points).  Outputs:
 *   y_out (npts, nullable)        gpry_predict of the point, bit for bit, clip and gates included (a gated point is -inf);
 *   G_out (npts x p, row-major)   the derivative of the UNCLIPPED, UNGATED mean, in units of y per unit of log theta;
 *                                 finite for a gated point too.
 * The bits of y and G depend on the model and the point alone: not on npts, the point's position in the batch, how a
 * batch is split over calls, or the context.  W is recomputed by every call (fixed summation orders: its bits depend on
 * the model alone); nothing is cached across calls.
 * Refused (-1, with gpry_last_error) before anything runs: a NULL X or G_out; npts < 1; no valid factor; d > 32; a
 * coordinate that is not finite.  After a refusal the context answers the next call as before.
 * State contract: works on a factor grown by gpry_append_rows; stops the resident predict kernel first; reads V, alpha_,
 * the scaled training rows, y_ and the noise vector only; writes a scratch of its own (2 Np 40 doubles, released with the
 * context) and the samplers' staging buffer.  The state of gpry_predict, a sweep, a Kriging-believer session, the
 * samplers, the buffers of gpry_loo and the factor cache of gpry_lml are not touched.  Stage timers: "theta_grad_setup"
 * (U, T = V U, W = V^T T), "theta_grad" (the points, once per chunk).  device_ms (nullable): device time of the call, copies
 * included. */
int gpry_mean_theta_grad(gpry_ctx* ctx, const double* X, int64_t npts, double* y_out, double* G_out, double* device_ms);

/* ---- The posterior mean at M points under B thetas, without touching the model the context holds (predict_thetas.hip;
 * gpry_amd/gpr.py: predict_thetas, gpry_amd/hyper.py: hyper_spread(exact=True)).
 * thetas: B rows of n_theta entries laid out as for gpry_lml_batch ([log C, log l_1 .. l_d], log w last with
 * GPRY_KERNEL_WHITE; every row has its own w); the kernel family is the context's, as given to gpry_set_theta (all four
 * ids).  X (M x d, raw coordinates where the affine map has an x-affine, as for gpry_mean_theta_grad).  B and M are
 * unbounded: the thetas go through in chunks of scratch sets (the arena of gpry_lml_batch), the points in chunks of 65536.
 *   mean (B x M, row-major)   mean[b M + i] = y_mean + y_std k_b(x_i)^T alpha_b, alpha_b = (C_b phi_b + diag(alpha + w_b))^-1 y_:
 *                             the UNCLIPPED, UNGATED mean in untransformed units (what G_out of gpry_mean_theta_grad
 *                             differentiates); a point so far away that k underflows gives exactly y_mean;
 *   lml (B, nullable)         gpry_lml(theta_b, want_grad = 0), bit for bit;
 *   info (B, nullable)        gpry_lml's convention: a theta whose matrix is not positive definite has info > 0, lml = -inf
 *                             and a row of NaN in mean, on its own -- the other rows are unaffected.
 * Up to the "lml_batch" limit one chain of launches (covariance build, factor, alpha_, log-determinant) carries all thetas
 * of a chunk, each in a scratch set of its own, always in the latency schedule (option "lml_schedule" is not read); one
 * kernel then evaluates every (theta, point) of the chunk, four points per workgroup.  Above the limit, with the rocSOLVER comparator, where fewer
 * than two sets fit, with one theta and at 128 padded rows the thetas go one after another through the same chain and the
 * same kernel in the context's own scratch.
 * The bits of mean[b, i] and lml[b] depend on the model, theta_b and x_i alone: not on B, M, the row's or the point's
 * position, how thetas or points are chunked or split over calls, the route, option "lml_batch_mb" or the context.  A
 * point is evaluated with the arithmetic of gpry_predict's one-point path: mean[b, i] has the bits of gpry_predict(x_i[None])
 * on a context factorised at theta_b with the clip off and no gates (gpry_predict's other paths have bits of their own).
 * Refused (-1, with gpry_last_error) before anything runs: NULL thetas, X or mean; B < 1 or M < 1; no training set or no
 * kernel id; a theta entry or a coordinate that is not finite; d > 32.  After a refusal the context answers the next call
 * as before.
 * State contract: that of gpry_lml_batch -- borrows the batch arena, the scratch of the objective and the samplers' staging
 * buffer, disarms the factor cache of gpry_lml, stops the resident predict kernel first.  The prediction factor and the
 * context's theta, a sweep, a Kriging-believer session, the gates, the buffers of gpry_loo and the scratch of
 * gpry_mean_theta_grad are not touched.  Stage timers: "predict_thetas" (a chunk's chain), "predict_thetas_mean" (the
 * point kernel).  device_ms (nullable): device time of the call, copies included. */
int gpry_predict_thetas(gpry_ctx* ctx, const double* thetas, int64_t B, const double* X, int64_t M, double* mean, double* lml,
                        int* info, double* device_ms);

/* ---- ... and the predictive variance beside it: what the error bar at x is made of once theta is marginalised
 * (predict_thetas.hip; gpry_amd/gpr.py: predict_thetas(return_std=True), gpry_amd/hyper.py: hyper_predict).
 * gpry_predict_thetas with one more output; with var NULL it IS gpry_predict_thetas.
 *   var (B x M, row-major, nullable)   var[b M + i] = y_std^2 (C_b + w_b - |V_b k_b(x_i)|^2), V_b = L_b^-1, w_b = 0 without a
 *                             white term: the prior variance of a new point at theta_b minus what the data explain, in
 *                             untransformed units.  NOT clamped at 0 -- rounding near a training point may leave a tiny
 *                             negative number (the convention of gpry_predict_cov's diagonal).  A theta with info > 0 has a
 *                             row of NaN, on its own; a point so far away that k underflows gives exactly y_std^2 (C_b + w_b).
 * mean, lml and info come from the kernels of gpry_predict_thetas and have its bits.  Per panel of points (as many as
 * fit, with their partial sums, into the third N x N piece of a theta's scratch set: about Np of them) three launches
 * carry all thetas of the chunk: the cross-kernel panel K*_b, the lower-triangular product V_b K*_b by the FP64 MFMA
 * engine of gemm_f64.hip with the column sums of squares taken in its epilogue (the product is never stored), and the
 * finish.  The route that takes the thetas one after another makes the same launches for one theta.
 * The bits of var[b, i] depend on the model, theta_b and x_i alone: not on B, M, the row's or the point's position, the
 * other points, how thetas or points are chunked or split over calls, the route, option "lml_batch_mb" or the context.
 * They are not the bits of any of gpry_predict's standard deviations (which differ among themselves).
 * Entry checks, refusals and the state contract are those of gpry_predict_thetas; the only scratch beyond its own is that
 * third piece of the scratch sets it borrows anyway, and as much again of the samplers' staging buffer.  Stage timers:
 * those of gpry_predict_thetas, "predict_thetas_var" (the three kernels, per chunk of points) and, inside it,
 * "predict_thetas_contract" (the matrix-pipe product alone, per panel; what tools/time_predict_thetas_var.py takes the
 * contraction's rate from). */
int gpry_predict_thetas_var(gpry_ctx* ctx, const double* thetas, int64_t B, const double* X, int64_t M, double* mean, double* var,
                            double* lml, int* info, double* device_ms);

/* ---- Predictions without a group of training points (predict_without.hip; gpry_amd/gpr.py: predict_without; the report in
 * gpry_amd/mc.py: batch_influence).  What the surrogate would predict at the M rows of X (raw coordinates where the affine
 * map has an x-affine, as for gpry_mean_theta_grad) had group g = idx[offsets[g] .. offsets[g + 1]) never been bought:
 * gpry_leave_out's groups (1 to 64 distinct indices in [0, N), groups may overlap, sorted on the host), at the current theta,
 * y map, noise vector and white term -- nothing is refitted.  With B = (K^-1)_GG = L_B L_B^T, W = L_B^-1 (the arithmetic,
 * and the bits, of gpry_leave_out), t = W alpha_G, S = W (V_G^T V) and s = S k*(x):
 *   dmean[g, i] = mean_-G(x_i) - mean(x_i) = -y_std s.t        of the UNCLIPPED, UNGATED mean, units of y;
 *   dvar[g, i]  = var_-G(x_i) - var(x_i)   = +y_std^2 |s|^2    of the latent variance, units of y^2: a sum of squares, >= 0
 *                 (the prior variance C + w cancels: nothing is clamped);
 *   info[g]     gpry_leave_out's: non-zero where B is not positive definite; that group's rows are NaN, the others unaffected.
 * dmean, dvar: ngroups x M row-major, either may be NULL; info and device_ms nullable.  All four kernels, GPRY_KERNEL_WHITE,
 * factors grown by gpry_append_rows, models below 128 rows.  No factorisation: per group one n x N x N / 2 product on the FP64
 * matrix pipe, per point and group n N multiply-adds beside the kernel row (the stacked rows of up to 64 groups against a
 * panel of 2048 points, on the matrix pipe).  M is unbounded (panels of 2048 points, uploads of 32768).
 * dmean[g, i] and dvar[g, i] depend bit for bit on the model, the group as a set and the point alone: not on M, the point's
 * position, how points or groups are split over calls, panels or batches, the other groups, the group's place in the list or
 * the context.  A point whose k* underflows gives exactly 0 and 0.
 * Refuses (-1, gpry_last_error) before anything is launched: NULL idx / offsets / X; both outputs NULL; ngroups < 1; M < 1; no
 * valid factor; d > 32; a coordinate that is not finite; gpry_leave_out's group refusals (empty, above 64, out of range, an
 * index twice).  Stops the resident predict kernel first.  Reads V, alpha_ and the scaled training rows; writes a scratch of
 * its own (sized as predict_without.hip states, released with the context, and by gpry_set_train below half the model size it
 * served) and the staging buffer: gpry_predict's state, a sweep, a Kriging-believer session, the samplers, gpry_loo's buffers
 * and gpry_lml's factor cache are untouched.  Stage timers "without_setup", "without_points" and, inside the latter,
 * "without_panel" and "without_contract". */
int gpry_predict_without(gpry_ctx* ctx, const int64_t* idx, const int64_t* offsets, int64_t ngroups, const double* X, int64_t M,
                         double* dmean, double* dvar, int* info, double* device_ms);

/* ---- The derivative of the latent predictive variance in theta at a batch of points (var_theta_grad.hip; gpry_amd/gpr.py:
 * var_theta_grad, gpry_amd/hyper.py: hyper_acq_spread).  theta, K, h, diff and dk_ia = d k_i / d log l_a = C h(r_i) diff_ia^2 as
 * for gpry_mean_theta_grad, at the theta of the factor the context holds; dK_a = dK / dlog l_a is the same expression between
 * training rows (zero diagonal).  With k = k*(x), t = V k, q = K^-1 k = V^T t and var(x) = y_std^2 (C + w - |t|^2):
 *   G_0(x) = y_std^2 ((C - |t|^2) - sum_i (alpha_i + w) q_i^2)        log C
 *   G_a(x) = y_std^2 (-2 sum_i q_i dk_ia + q^T dK_a q)                log l_a
 *   G_w(x) = y_std^2 w (1 + |q|^2)                                    log w
 * The log C entry uses q^T (C phi) q = q^T k - q^T diag(alpha + w) q and is formed as written, never as C - 2 k^T q + q^T (C phi) q,
 * which cancels to nothing next to a training point.  No factorisation: once per call the d matrices dK_a among the training
 * rows (the pairs kernel of gpry_lml_hessian), then per panel of gpry_var_theta_grad_panel(ctx) points the cross-kernel panel of
 * gpry_predict_thetas_var, T = V K* and Q = V^T T over the triangular k-ranges of the FP64 MFMA engine of gemm_f64.hip, the d
 * products dK_a Q in one batched launch of the same engine and one FP64 vector kernel that forms the sums above per point:
 * (2 + 2 d) N^2 flop per point on the matrix pipe.
 * X (npts x d, raw coordinates where the affine map has an x-affine, as for gpry_mean_theta_grad); npts is unbounded (panels
 * inside chunks of 65536 points).  Outputs:
 *   var_out (npts, nullable)      y_std^2 (C + w - |V k|^2), the latent variance of gpry_predict_thetas_var: not clamped at 0,
 *                                 not clipped, not gated;
 *   G_out (npts x p, row-major)   d var / d theta in units of y^2 per unit of log theta; finite everywhere.  A point so far away
 *                                 that k underflows gives exactly [y_std^2 C, 0 .., y_std^2 w].
 * Every sum has a fixed order: the bits of var and G depend on the model and the point alone, not on npts, the point's
 * position, the other points of its panel, how a batch is split over calls, or the context.  They are not the bits of any
 * other call's variance.
 * Refused (-1, with gpry_last_error) before anything runs: a NULL X or G_out; npts < 1; no valid factor; d > 32; a model above
 * 4096 padded rows (d squares of scratch, gpry_lml_hessian's limit); a coordinate that is not finite.  After a refusal the
 * context answers the next call as before.
 * State contract: works on a factor grown by gpry_append_rows; stops the resident predict kernel first; reads V, the scaled
 * training rows, the noise vector and the affine map only; writes a scratch of its own (d Np^2 doubles for the dK_a and
 * (3 + d) Np pc and the row slices' sums for a panel of pc <= gpry_var_theta_grad_panel(ctx) points, released with the context, and by gpry_set_train when
 * the model falls below half the footprint it was sized for) and the samplers' staging buffer.  The state of gpry_predict, a
 * sweep, a Kriging-believer session, the gates, the scratch of gpry_lml_hessian, gpry_mean_theta_grad, gpry_loo and
 * gpry_predict_without and the factor cache of gpry_lml are not touched.  Stage timers: "var_theta_grad_setup" (the dK_a),
 * "var_theta_grad" (a panel) and, inside it, "var_theta_grad_panel", "var_theta_grad_solve" (T and Q),
 * "var_theta_grad_products" (the batched launch) and "var_theta_grad_finish".  device_ms (nullable): device time of the
 * call, copies included. */
#define GPRY_VAR_THETA_GRAD_PANEL 1024      /* the narrowest panel */
int gpry_var_theta_grad(gpry_ctx* ctx, const double* X, int64_t npts, double* var_out, double* G_out, double* device_ms);
/* points per panel of gpry_var_theta_grad for the model the context holds, a function of its padded size alone: 4096 up to
 * 1024 padded rows, 2048 up to 2048, GPRY_VAR_THETA_GRAD_PANEL above (and for a NULL context) */
int64_t gpry_var_theta_grad_panel(gpry_ctx* ctx);

/* ---- f3: x-gradients for one point (gpry/gpr.py:1236-1266) ------------------------- */
/* x: d doubles, raw/transformed as in gpry_predict.  With G[j][k] = d k(x, X_j) / d x_k in the
 * kernel's coordinates (kernel_.gradient_x: gpry/kernels.py:257-278 RBF, :326-432 Matern,
 * :687-699 product), returns
 *   kgrad      (nullable, N x d)  G
 *   mean_grad  (nullable, d)      G^T alpha_                  -> grad_mean = std_y * mean_grad
 *   kinvk_grad (nullable, d)      G^T K^-1 k*(x), if want_kinv -> grad_std = -std_y^2 * kinvk_grad / sigma_
 * in transformed units; the y-scalings (once for the mean, twice for the std, as the
 * reference does) are left to the caller. */
int gpry_predict_grad(gpry_ctx* ctx, const double* x, int want_kinv, double* kgrad,
                      double* mean_grad, double* kinvk_grad);

/* The same for m points in one call (m <= 4096): V is read once for all of them (two triangular
 * products on the MFMA engine) instead of twice per point.  What a batch of acquisition-optimiser
 * restarts evaluated side by side needs (gpry/gp_acquisition.py:270-389 runs them one after another,
 * each step = one predict with gradients).  mean / std (nullable, m each): as gpry_predict without a
 * mask; mean_grad, kinvk_grad: m x d, transformed units as above. */
int gpry_predict_grad_batch(gpry_ctx* ctx, const double* X, int64_t m, int want_kinv, double* mean,
                            double* std, double* mean_grad, double* kinvk_grad);

/* ONE point, everything in one call: what gpry/gpr.py:1022-1273 returns for predict(x, return_std=True,
 * return_mean_grad=True[, return_std_grad=True]) -- the call the acquisition optimiser makes once per L-BFGS step
 * (gpry/gp_acquisition.py:309-342, gpry/acquisition_functions.py:937-1009).  mean / std as gpry_predict finalises them
 * (y map, clipping; mask_bits: GPRY_MASK_* verdicts of the caller for this point: mean -inf, and std 0 for the
 * classifier bit; with option "predict_gates" the device's own verdict of gpry_set_gates is ORed in; *verdict (nullable)
 * returns the bits that were applied), mean_grad / kinvk_grad (d each; kinvk_grad only with want_kinv) as gpry_predict_grad.  Four launches
 * and one stream wait instead of gpry_predict + gpry_predict_grad (seven launches, two copies, two waits). */
int gpry_predict_point(gpry_ctx* ctx, const double* x, int mask_bits, int want_kinv, double* mean, double* std,
                       double* mean_grad, double* kinvk_grad, int* verdict);

/* ---- f4: gates of the sweep evaluated on the device --------------------------------- */
/* Replaces the host-side verdicts that gpry/gpr.py:1107-1112 (trust region, raw coordinates,
 * closed box) and :1145-1150 -> gpry/svm.py:308-347 (sklearn SVC, RBF kernel, two classes:
 * libsvm _dense_predict on the TRANSFORMED coordinates) compute per candidate.  Once set,
 * gpry_sweep_logexp ORs GPRY_MASK_OUTSIDE_TRUST / GPRY_MASK_CLASSIFIED_INF into the mask itself:
 *   finite  <=>  (sum_i coef[i] exp(-gamma |x_ - sv[i]|^2) + intercept > 0) == positive_is_finite
 * sv: n_sv x d support vectors, coef: dual_coef_[0], intercept: intercept_[0] of the fitted SVC;
 * trust_bounds: d x 2 (lo, hi) or NULL.  n_sv = 0 and trust_bounds = NULL switch the gates off.
 * gpry_predict keeps to the caller's mask unless the option "predict_gates" = 1 asks it to OR the same verdicts in
 * (what the host mirror does: the one-point calls of the samplers then cost no libsvm call each; the resident
 * kernel evaluates decision function and trust box next to the mean). */
int gpry_set_gates(gpry_ctx* ctx, const double* sv, const double* coef, int64_t n_sv, double gamma,
                   double intercept, int positive_is_finite, const double* trust_bounds);

/* ---- f4: training of that classifier on the device (svm_fit.hip) -------------------- */
/* What gpry/svm.py:227 leaves to sklearn's SVC, i.e. to libsvm (svm.cpp: Solver::Solve, select_working_set,
 * calculate_rho): the C-SVC dual of two classes with the RBF kernel k(a, b) = exp(-gamma |a - b|^2),
 *   minimise 1/2 alpha^T Q alpha - sum alpha,  0 <= alpha_t <= C,  sum y_t alpha_t = 0,  Q_ts = y_t y_s k(x_t, x_s),
 * y_t = +1 where finite[t] != 0 ("finite") and -1 elsewhere, by sequential minimal optimisation.  X: N x d row-major, in
 * the coordinates the classifier is evaluated in (the TRANSFORMED ones of gpry_set_gates).  The gradient G = Q alpha - e is
 * kept incrementally.  Per iteration, as libsvm's second-order rule (WSS 2):
 *   i = argmax of -y_t G_t over I_up = {y_t = +1, alpha_t < C} U {y_t = -1, alpha_t > 0}, G_max its value;
 *   j = argmin of -b^2 / a over t in I_low = {y_t = +1, alpha_t > 0} U {y_t = -1, alpha_t < C} with b = G_max + y_t G_t > 0,
 *       a = 2 - 2 k(x_i, x_t), a non-positive a replaced by tau = 1e-12; G_min = min of -y_t G_t over I_low;
 *   stop when G_max - G_min < eps; else libsvm's two-variable update of (alpha_i, alpha_j) with its four clipping branches
 *   and G_t += Q_ti d alpha_i + Q_tj d alpha_j.
 * Not libsvm's: no shrinking; a TIE in either selection goes to the SMALLEST index (libsvm's scan keeps the last one);
 * and convergence is declared on a gradient without the rounding of the steps: when the stop test passes, G is recomputed
 * from alpha (per point the rows with alpha > 0 in ascending index order) and the test repeated on it; if it fails there
 * the iteration goes on from the recomputed gradient.  r^2 is the sum of the squared coordinate differences in coordinate
 * order and the exponential is the routine of the device's gates, so the trained function and its evaluation by
 * gpry_set_gates see the same kernel values.
 * Outputs: alpha (N); *rho as calculate_rho (the mean of y_t G_t over the free variables 0 < alpha_t < C, the midpoint of
 * the two bounds when there is none): decision(x) = sum_t y_t alpha_t k(x_t, x) - rho, finite <=> decision > 0, i.e.
 * gpry_set_gates(sv = the rows with alpha > 0, coef = y alpha, intercept = -rho, positive_is_finite = 1); *objective =
 * 1/2 sum alpha_t (G_t - 1); *violation = G_max - G_min of the last stop test; *n_iter the updates made; *status 0 =
 * converged, 1 = max_iter updates were made first (alpha is feasible all the same; not an error).  rho, objective,
 * violation, n_iter, status and device_ms may be NULL.
 * One workgroup runs the solve (the method is serial), at most "svm_iters_per_launch" updates per launch (option, default
 * 4096; a launch is finite, the state -- alpha, G, a status block -- stays in device memory between launches); kernel rows
 * are kept in an on-demand cache of up to 32 MB in device memory (a cached row is the computed row bit for bit).  The bits
 * of every output depend on (X, finite, C, gamma, eps, max_iter) alone: not on the context, on that option, or on what
 * else the context holds.  Refuses (-1, gpry_last_error) N < 2, N > 8192, d > GPRY_MAX_DIM, labels of one class,
 * non-finite X, and C, gamma or eps that are not positive and finite.  Stops the resident predict kernel first and
 * touches nothing else: model, factor, sweep, gates, Kriging-believer session and samplers stay as they are.  Stage timer
 * "svm_fit"; device_ms: device time of the call, copies included. */
int gpry_svm_fit(gpry_ctx* ctx, const double* X, const uint8_t* finite, int64_t N, int64_t d, double C, double gamma,
                 double eps, int64_t max_iter, double* alpha, double* rho, double* objective, double* violation,
                 int64_t* n_iter, int* status, double* device_ms);

/* ---- a8-a13: fused NORA sweep ----------------------------------------------------- */
/* For all M candidates: mean, std (as gpry_predict), acq = LogExp.f(mean, std,
 * baseline, sigma_n, zeta) (gpry/acquisition_functions.py:1068-1074), kept resident on
 * the device; y_all / sigma_all / acq_all (nullable) receive host copies.
 * n_nan receives the number of NaN acquisition values (the reference raises on those,
 * gpry/gp_acquisition.py:1453-1455). */
int gpry_sweep_logexp(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask,
                      double zeta, double baseline, double sigma_n,
                      double* y_all, double* sigma_all, double* acq_all,
                      int64_t* n_nan);
/* The sweep of a pool whose sampler supplied y, or y and sigma_y (NORA._set_MC_sample, gpry/gp_acquisition.py:858-873 ->
 * mpi.compute_y_parallel, gpry/mpi.py:182-218; the acquisition is LogExp.f on those arrays, gp_acquisition.py:1049-1054).
 * y_given (M values) is required; X == NULL re-uses the resident pool as in gpry_sweep_logexp.
 *   sigma_given == NULL: y is the caller's as it is -- no y map, no clip, and a masked row does NOT get -inf; sigma is
 *     gpr.predict_std (gpry/gpr.py:1275-1352): exactly the sigma of gpry_sweep_logexp on the same pool (same panel form,
 *     contraction and per-tile summation order), 0 where GPRY_MASK_CLASSIFIED_INF is set.  predict_std has no trust-region
 *     gate: GPRY_MASK_OUTSIDE_TRUST (the caller's or the device gates') changes neither y nor sigma, and such a row keeps a
 *     finite acquisition.  acq = LogExp.f(y_given, sigma).  Option "sweep_prune" with no arrays wanted: the bound of every
 *     candidate comes from y_given and the prior sigma, without a mean pass; gpry_sweep_topk / gpry_sweep_fetch then work as
 *     after a pruned gpry_sweep_logexp.
 *   sigma_given != NULL: acq = LogExp.f(y_given, sigma_given) and nothing else -- no panel, no contraction, no gates, no mask
 *     (mask is ignored).  No factor is needed (the rows of X need the width of gpry_set_train).
 * y_all / sigma_all / acq_all / n_nan and the resident arrays as for gpry_sweep_logexp: gpry_sweep_fetch and
 * gpry_sweep_topk work unchanged on them. */
int gpry_sweep_logexp_given(gpry_ctx* ctx, const double* X, int64_t M, const uint8_t* mask,
                            const double* y_given, const double* sigma_given,
                            double zeta, double baseline, double sigma_n,
                            double* y_all, double* sigma_all, double* acq_all,
                            int64_t* n_nan);
/* How the cross-kernel panel K(X*, X_train) (gpry/gpr.py:1179) of the context's last sweep / panel predict was built, and the
 * error estimates of the model that decided it.  *panel_form: 0 none yet, 1 distances from the matrix pipe (expanded form
 * |x|^2 + |y|^2 - 2 x.y on centred coordinates), 2 difference form (as scipy's cdist), 3 the small-batch kernel (difference
 * form), 4 hybrid: distances from the matrix pipe, every pair nearer than r^2 = 100 again from the coordinates (taken by a model
 * that fails the gate of form 1 through length scales far below the extent of its data; option "cross_hybrid").  est[0]: estimated error of the posterior mean in units of the normalised targets (entry error x ||alpha_||_2);
 * est[1]: its worst case (x ||alpha_||_1); est[2]: estimated error of the posterior variance relative to the prior
 * variance C (2 x entry error x the bound sqrt(C) / sigma_n,min of ||K^-1 k*||_2); est[3]: the gate both est[0] and est[2]
 * must stay below for form 1 (2.5e-7, a quarter of the 1e-6 the posterior is specified to).  Either pointer may be NULL. */
int gpry_sweep_info(gpry_ctx* ctx, int* panel_form, double* est);
/* Host copies of the arrays of the last gpry_sweep_logexp that are still resident on the device
 * (any pointer may be NULL; M must be the size of that sweep).  Lets a caller skip the copies in
 * gpry_sweep_logexp and fetch them only if somebody asks (NORA.last_MC_sample). */
int gpry_sweep_fetch(gpry_ctx* ctx, int64_t M, double* y_all, double* sigma_all, double* acq_all);
/* Shortlist of the last sweep: the Kp candidates with the largest acq in the total
 * order (acq desc, idx desc) -- the order of np.argsort(acq)[::-1] on distinct values
 * (gpry/gp_acquisition.py:1328-1329).  exclude (nullable, n_exclude sorted indices):
 * rows dropped as "already proposed" (gpry/gp_acquisition.py:1037-1047).
 * *n_out <= Kp records written, sorted; *bound = largest acq NOT returned (-inf if
 * none): every candidate outside the shortlist has acq <= *bound.
 * After a pruned sweep (option "sweep_prune") the records are those of the full sweep, bit for bit, and *bound is >= the
 * full sweep's bound: the largest acq not returned, or the largest upper bound of a candidate that was never contracted.
 * gpry_sweep_fetch after a pruned sweep runs the full sweep first. */
int gpry_sweep_topk(gpry_ctx* ctx, int64_t Kp, const int64_t* exclude, int64_t n_exclude,
                    gpry_cand* top, int64_t* n_out, double* bound);
/* Statistics of the last pruned sweep: info[0] 1 while it is still pruned (0 once completed or after a full sweep),
 * [1] pool size, [2] candidates ranked by bound and contracted exactly (K'), [3] contraction rounds, [4] candidates
 * contracted in all, [5] 1 if the full sweep had to run, [6] Kp of the last gpry_sweep_topk, [7] candidates whose bound
 * was not below the threshold of the first contraction round (-1: that round answered alone), [8] 1 if the mean pass bounded y
 * (option "sweep_mean_bound"): the survivors of [7] were then ranked by bounds of y as well, [9] blocks of 16 training rows x
 * 32 candidates that pass evaluated, [10] blocks it saw (info: 11 values).  dinfo (nullable, 5 doubles):
 * [0] that threshold (NaN if none), [1..4] device ms so far of the stages "sweep_mean", "sweep_prune_select", "sweep_compact",
 * "sweep_prune_gemm" (the per-stage timers of gpry_timing_get; 0 while timing is off).  The contraction rounds and the
 * completion use a copy of the model taken at the end of the sweep: a refit or refactorisation in between does not change
 * what they compute. */
int gpry_sweep_prune_info(gpry_ctx* ctx, int64_t* info, double* dinfo);
/* The FP32 screen of that mean pass (option "sweep_screen") in the last pruned sweep: out[0] blocks it certified as skipped
 * without the FP64 test, out[1] blocks the pass saw ([10] above).  out[0] <= [10] - [9]; 0 where the pass did not bound y. */
int gpry_sweep_screen_info(gpry_ctx* ctx, int64_t out[2]);

/* ---- a14/a15: Kriging-believer support (bordered factor instead of deepcopy+refit) - */
/* Start a session on the current factor; drops any registered candidates. */
int gpry_kb_reset(gpry_ctx* ctx);
/* Register m candidates (X: m x d, raw/transformed as in gpry_predict): computes and
 * keeps u(x) = V k*(x).  They get session indices [*first, *first + m).  var0 (nullable)
 * receives C - |u|^2 (transformed units, unclamped). */
int gpry_kb_register(gpry_ctx* ctx, const double* X, int64_t m, int64_t* first,
                     double* var0);
/* For registered candidate p: G[x] = u(p).u(x) and kvec[x] = kernel_(x_p, x) for every
 * registered x (n = number registered so far; both arrays length n). */
int gpry_kb_gram(gpry_ctx* ctx, int64_t p, double* G, double* kvec, int64_t* n);
/* The same for n_rows registered candidates p[] in ONE launch: row j of G / kvec (n_rows x n, row-major) is what
 * gpry_kb_gram(p[j]) returns, bit for bit, whatever shares the launch. */
int gpry_kb_gram_rows(gpry_ctx* ctx, const int64_t* p, int64_t n_rows, double* G, double* kvec, int64_t* n);
/* The Kriging-believer ranking of an offer in one call: RankedPool.add(method="single sort acq") with add_one,
 * _position_for, sort, cache_model and the conditioned models' predict_std (gpry/gp_acquisition.py:1290-1335, 1392-1520,
 * 1522-1555, 1598-1670), for a model without infinities classifier and with a scalar noise level.  The slot logic runs on
 * the host (csrc/kb_rank_core.h, which writes down the order of operations); the Gram rows it needs come from batched
 * launches, the first of them speculative (the pool's slots and the first 2 n_points offers in walking order).
 *   X_new (m_new x d): the offer's rows that the session does not hold yet; they are registered first (gpry_kb_register)
 *     and get the session indices [n_session - m_new, n_session).  var0 (n_session): C - |u|^2 of every session candidate;
 *     the last m_new entries are written here.
 *   idx, y, sigma, acq (n_offer): session index and sweep values of each offered row; order (n_order): the walk,
 *     np.argsort(acq)[::-1] of the caller.  params: sigma_n, alpha (noise on the border diagonal, transformed units),
 *     baseline, zeta, y_std.
 *   slot_* (n_points + 1 each, in/out) and *cache_counter (in/out): the pool; slot_idx -1 = never filled, slot_acq_cond
 *     -inf = empty.  A second call continues the pool.
 *   *info: 0, or t + 1 when the t-th appended point makes the augmented kernel matrix non positive definite (the pool is
 *     then left as it stood at that point).  stats (nullable, 3 values): Gram launches, rows fetched, requests of the core
 *     beyond the speculative one.
 * Against the Python path only the rounding inside slot_acq_cond may differ (numpy's dot sums in BLAS order). */
int gpry_kb_rank(gpry_ctx* ctx, const double* X_new, int64_t m_new, double* var0, int64_t n_session,
                 const int64_t* idx, const double* y, const double* sigma, const double* acq, int64_t n_offer,
                 const int64_t* order, int64_t n_order, const double* params, int64_t n_points,
                 int64_t* slot_idx, double* slot_y, double* slot_sigma, double* slot_acq, double* slot_acq_cond,
                 int64_t* cache_counter, int64_t* info, int64_t* stats);

/* ---- a16: multi-GPU (one process per GPU, RCCL over xGMI) -------------------------- */
/* 128-byte RCCL unique id, made on rank 0 and distributed by the caller. */
int gpry_comm_unique_id(uint8_t id[128]);
int gpry_comm_init(gpry_ctx* ctx, int world, int rank, const uint8_t id[128],
                   gpry_comm** out);
int gpry_comm_destroy(gpry_comm* comm);
/* what RCCL itself reports for this communicator: ncclCommCount / ncclCommUserRank / ncclCommCuDevice
 * (any pointer may be NULL).  bench.py prints the count as config.rccl_ranks. */
int gpry_comm_info(gpry_comm* comm, int* world, int* rank, int* device);
/* all-gather of `bytes` host bytes per rank (staged through device buffers, RCCL) */
int gpry_comm_allgather(gpry_comm* comm, const void* send, int64_t bytes, void* recv);
/* all-reduce(max) of n doubles */
int gpry_comm_allreduce_max(gpry_comm* comm, double* inout, int64_t n);
int gpry_comm_barrier(gpry_comm* comm);

/* ---- a16: single-process device group (k contexts behind one call) ------------------ */
/* What an unmodified gpry.Runner needs to use several GPUs: it is ONE Python process (mpi4py absent
 * => 1-rank dummy, gpry/mpi.py:18-28) that calls multi_add once per iteration (gpry/run.py:838-844).
 * A group holds n contexts on devices[0..n) (entries may repeat: several contexts on one GPU) and
 * drives them from n host threads inside each call.  Partitioning and merge are those of the
 * one-process-per-GPU path: contiguous candidate shards [i*ceil(M/n), ...), model replicated and
 * factorised on every member (gpry/mpi.py:105-131,182-218 shard X[rank::SIZE] and gather instead),
 * shortlists merged with the hold-back rule that keeps the descending stream exact
 * (gpry/gp_acquisition.py:1148-1191 merges per-rank pools).  adopt0 (nullable): an existing context
 * on devices[0] becomes member 0 and stays owned by the caller (it must hold the factorised model;
 * gpry_group_set_model leaves it alone).  The shortlist records (a few KB that the host ranks) are
 * copied out by every member and merged on the host (transport 0); with GPRY_GROUP_TRANSPORT=rccl and
 * all devices distinct they travel by an in-process RCCL all-gather instead (ncclCommInitAll;
 * transport 1; falls back to 0, with the reason in the error text, if RCCL declines). */
int gpry_group_create(int n, const int* devices, gpry_ctx* adopt0, gpry_group** out);
int gpry_group_destroy(gpry_group* group);
int gpry_group_size(gpry_group* group, int* n, int* transport);
gpry_ctx* gpry_group_member(gpry_group* group, int i);     /* for per-member options / timers */
const char* gpry_group_last_error(gpry_group* group);
/* gpry_set_train + gpry_set_theta + gpry_set_affine + gpry_factorize on every owned member,
 * concurrently; *info = first non-zero factorisation status. */
int gpry_group_set_model(gpry_group* group, const double* X_, const double* y_, const double* alpha,
                         int64_t N, int d, int kernel_id, const double* theta, const gpry_affine* tf,
                         int* info);
/* gpry_set_gates on every member (adopted one included) */
int gpry_group_set_gates(gpry_group* group, const double* sv, const double* coef, int64_t n_sv,
                         double gamma, double intercept, int positive_is_finite,
                         const double* trust_bounds);
/* gpry_sweep_logexp over the whole pool, member i on rows [lo_i, hi_i); arguments as there (host
 * arrays of M rows; X == NULL re-uses the resident shards).  gpry_group_sweep_fetch likewise. */
int gpry_group_sweep_logexp(gpry_group* group, const double* X, int64_t M, const uint8_t* mask,
                            double zeta, double baseline, double sigma_n, double* y_all,
                            double* sigma_all, double* acq_all, int64_t* n_nan);
/* gpry_sweep_logexp_given over the whole pool likewise: member i gets rows [lo_i, hi_i) of y_given (and sigma_given). */
int gpry_group_sweep_logexp_given(gpry_group* group, const double* X, int64_t M, const uint8_t* mask,
                                  const double* y_given, const double* sigma_given,
                                  double zeta, double baseline, double sigma_n, double* y_all,
                                  double* sigma_all, double* acq_all, int64_t* n_nan);
int gpry_group_sweep_fetch(gpry_group* group, int64_t M, double* y_all, double* sigma_all,
                           double* acq_all);
/* Global shortlist: every member selects its Kp best (gpry_sweep_topk, exclusions = sorted GLOBAL
 * rows), the records are merged in the total order (acq desc, idx desc, idx global) and entries
 * with acq <= max_i bound_i are held back unless every member was exhausted.  top must hold
 * n * Kp records; *bound = largest acq that may be missing from the returned prefix (-inf if the
 * pool is exhausted), *exhausted (nullable) = 1 if every member returned fewer than Kp. */
int gpry_group_sweep_topk(gpry_group* group, int64_t Kp, const int64_t* exclude, int64_t n_exclude,
                          gpry_cand* top, int64_t* n_out, double* bound, int* exhausted);
/* n_theta independent LML (+gradient) evaluations, theta t on member t mod n, members concurrently
 * (restart farm, gpry/run.py:1252-1293: independent start points).  thetas: n_theta x (1+d);
 * grad: n_theta x (1+d); info: n_theta (nullable).  Every member must hold the training set. */
int gpry_group_lml_batch(gpry_group* group, const double* thetas, int n_theta, int want_grad,
                         double* lml, double* grad, int* info);

/* ---- measurement ------------------------------------------------------------------ */
/* Device-side timing of the last call's stages in milliseconds (HIP events on the
 * ctx stream).  Known names: "kernel_build", "potrf", "trtri", "lauum", "lml_traces",
 * "cross_build", "sweep_gemm", "sweep_finish", "topk".  Returns <0 if unknown.
 * *count = launches accumulated since gpry_timing_reset.  "lml_batch_shrinks" is a counter, not a timer: *count = the times a
 * batched objective of this context halved its chunk after an out-of-memory answer (any other failure is returned to the caller).
 * "capacity_rows" / "capacity_cols" are sizes, not timers: *count = the training rows / padded columns the context's buffers hold
 * (they grow with the largest model the context has seen and never shrink).  "scratch_bytes": *count = the bytes of the
 * context's call scratch, the one device buffer that the entry points with private scratch (gpry_lml_hessian,
 * gpry_var_theta_grad, gpry_mean_theta_grad, gpry_predict_without, gpry_predict_cov / gpry_sample_joint, gpry_loo /
 * gpry_leave_out, gpry_svm_fit, gpry_ns_knn, gpry_ns_generation_phantoms) hold one at a time: the largest footprint any of
 * them has needed, 0 once gpry_set_train has given it back (a model with 2 Np^2 below the square of the padded size the
 * buffer last grew under).  "batch_set_doubles" / "batch_chunk": the last
 * batched objective of this context (gpry_lml_batch, gpry_loo_objective_batch) that ran as one chain -- *count = the doubles of
 * one theta's scratch set in its arena / the thetas one chain carried at the most (option "lml_batch_mb" holds
 * floor(mb * 2^20 / (8 * batch_set_doubles)) sets). */
int gpry_timing_reset(gpry_ctx* ctx);
int gpry_timing_get(gpry_ctx* ctx, const char* name, double* total_ms, int64_t* count);
/* Raw micro-benchmarks used by bench.py to quote measured peaks beside the spec:
 * kind 0: f64 MFMA 16x16x4 issue loop, compiler-allocated (AGPR) accumulators; `bytes` =
 *         workgroups per CU (1..8) -> *value = TFLOP/s  (measured 35-49: AGPR accumulators
 *         run the f64 MFMA well below rate, which is why the GEMM keeps them in VGPRs)
 * kind 2: the same loop with the accumulators pinned to VGPRs -> TFLOP/s (measured 77.1-77.7)
 * kind 1: HBM streaming copy of `bytes` -> *value = GB/s (read+write bytes / time)
 * kind 3: HBM streaming fill of `bytes`  -> *value = GB/s written */
int gpry_microbench(gpry_ctx* ctx, int kind, int64_t bytes, double* value);

/* ---- testing hook ------------------------------------------------------------------- */
/* Runs the FP64 MFMA GEMM engine on host matrices (unit test of the fragment layout).
 * C(MxN) op= A(MxK) B(KxN); a_trans: A given as K x M; b_trans: B given as N x K;
 * epi 0 store, 1 store -AB, 2 C -= AB, 3 per-128-row-tile column sums of squares
 * (C is then ceil(M/128) x N); kmode 0 full (see csrc/common.h for the others).
 * M, N, K must be multiples of 64.  tile_map: bits 0..7 the tile map, bits 8..11 a uniform split-K factor,
 * bits 16..27 > 0: a stream-K launch with segments of that many slab pairs (32 k; M, N multiples of 128). */
int gpry_debug_gemm(gpry_ctx* ctx, const double* A, const double* B, double* C, int M, int N,
                    int K, int a_trans, int b_trans, int epi, int kmode, int lower_only,
                    int tile_map);

/* The acquisition epilogue of the sweep on caller-given (mean, std) pairs, no model involved:
 * acq[i] = LogExp.f(mu[i], sigma[i], baseline, sigma_n, zeta) (gpry/acquisition_functions.py:1068-1074),
 * incl. the edge cases sigma <= sigma_n and mu = -inf (-> -inf). */
int gpry_debug_logexp(gpry_ctx* ctx, const double* mu, const double* sigma, int64_t n, double zeta,
                      double baseline, double sigma_n, double* acq);

#ifdef __cplusplus
}
#endif
#endif /* GPRY_HIP_H */
