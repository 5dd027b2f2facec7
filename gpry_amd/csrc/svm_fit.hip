// Training of the infinities classifier on the device: the kernels behind gpry_svm_fit (gpry/svm.py:227 -> sklearn SVC ->
// libsvm svm.cpp: Solver::Solve).  The C-SVC dual of two classes with the RBF kernel k(a, b) = exp(-gamma |a - b|^2),
//   minimise 1/2 a^T Q a - sum a,  0 <= a_t <= C,  sum y_t a_t = 0,  Q_ts = y_t y_s k(x_t, x_s),
// by sequential minimal optimisation with libsvm's second-order working-set selection (Solver::select_working_set), its
// two-variable update with the four clipping branches and its calculate_rho; no shrinking.  include/gpry_hip.h states
// the selection and tie rules; tests/tools/svm_smo_numpy.py is the same order of operations in numpy.
//
// The method is serial (an iteration depends on the one before it) and an iteration is small (two kernel rows, two
// arg-reductions, one update of the gradient), so it is latency-bound: ONE workgroup of 1024 threads runs the whole solve,
// as lml_small.hip and maxmean_kernel do for their serial methods.  Thread t owns the points t, t + 1024, ... (PPT of
// them, a template parameter: 1, 2 or 4 with 1024 threads, 16 with 512 threads above N = 4096, where 8 per thread did not
// fit the 128 registers that 16 waves on one CU leave each thread); their alpha, gradient and label stay in registers and
// every loop over them is unrolled.  The coordinates are read from a coordinate-major copy [dpad][Npad] in global memory (at most 2 MB: L2), a
// row's loads are coalesced and x_i / x_j come through a workgroup-uniform address.
//
// One iteration, three barriers:
//   every thread    best of its points for i                  -> wave tree (shuffles) -> one partial per wave in LDS | barrier
//   every wave      folds the partials (i, G_max); every thread gets row i of the kernel for its points and the best of its
//                   points for j -> wave tree -> partials; the lane that holds a wave's best adds that point's alpha,
//                   gradient, label and k_ij, the owner of i its alpha, gradient and label                          | barrier
//   wave 0          folds them (j, G_min); its first thread takes the stop decision, solves the two-variable problem and
//                   writes the control block                                                                        | barrier
//   every thread    reads the control block; on "go on" gets row j and updates its gradients; the owners of i and j
//                   take the new alphas.
// Every barrier sits in code all threads reach together: the loop's only exit depends on the control block, which one
// thread wrote.  No atomics, no spin waits, no traffic between workgroups.
//
// Kernel rows come through a row cache in device memory (svm_row_cached): SMO keeps returning to the support vectors,
// and a hit replaces d loads and an exponential per point by one load.  A row is stored the first time it is computed,
// while slots last (no eviction); each thread reads back only the entries it stored itself, and a cached row is the
// computed row bit for bit, so nothing depends on the cache but the time.  Which rows are cached is workgroup-uniform
// bookkeeping that every thread keeps alike; the table row -> slot sits in LDS, is written by thread 0 alone, between
// the second and the third barrier, and read by the others between the first and the second (row i; row j's slot comes
// with the control block).  The cache starts empty with every launch.
//
// Convergence is declared on a gradient WITHOUT the rounding of the steps: when the stop test passes on the incremental
// gradient the launch ends with state 1; gpry_svm_fit then recomputes G = Q alpha - e from alpha (svm_grad_kernel: a thread
// per point, the rows with alpha > 0 in ascending order) and launches again, marked "fresh".  A stop test that passes
// before any further step is final (state 2); one that fails goes on iterating from the recomputed gradient.
#include "common.h"
#include "kern_math.h"
#include "ns_common.h"
#include <algorithm>

#define SVM_MAX_WAVES 16
#define SVM_MAX_N 8192
#define SVM_TAU 1e-12
// keeps the scheduler from interleaving the two halves of a kernel row
#define SVM_SEQ() __builtin_amdgcn_sched_barrier(0)

struct SvmStatus {                  // device; the host's copy after every launch
    long long n_iter;               // steps taken so far (all launches)
    int state;                      // 0: the launch's budget ran out, 1: stop test passed on the incremental gradient, 2: on a fresh one
    int fresh;                      // in: the gradient was recomputed and no step has been taken since
    double rho, objective, gmax, gmin;
};

struct SvmPart { double v; int idx; int pad; double a, g, y, k; };     // a wave's best and that point's alpha, gradient, label, k_ij

struct SvmCtl { int stop, i, j, slot_j; double ai, aj, ci, cj; };       // slot of row j in the cache; new alphas; c = y * (new - old)

// (v, idx) <- the better of the two: larger v, equal v to the SMALLER index (idx < 0: no candidate)
__device__ __forceinline__ bool svm_better(double v, int idx, double bv, int bidx) {
    return idx >= 0 && (bidx < 0 || v > bv || (v == bv && idx < bidx));
}

__device__ __forceinline__ double svm_shfl(double x, int m) { return __shfl_xor(x, m, 64); }

// k(x_s, x_p) for the thread's points p = t + q T: r^2 is the sum of the squared differences in coordinate order (the zero
// padding adds exact zeros), the exponential is gates_kernel's.  At most four points at a time, so that the loads in flight
// and the partial sums of eight points do not meet in the register file.
template <int PPT, int SVM_T>
__device__ __forceinline__ void svm_row(const double* __restrict__ Xt, int Npad, int dpad, double gamma, int s, int t,
                                        double (&kr)[PPT]) {
    constexpr int PH = PPT < 4 ? PPT : 4;
#pragma unroll
    for (int h = 0; h < PPT; h += PH) {
        int tt = t;
        asm volatile("" : "+v"(tt));         // offsets formed per half, not eight of them carried through the iteration
        double r2[PH];
#pragma unroll
        for (int q = 0; q < PH; q++) r2[q] = 0.0;
#pragma unroll 2
        for (int k = 0; k < dpad; k++) {
            const double* row = Xt + (size_t)k * Npad;
            const double xs = row[s];
#pragma unroll
            for (int q = 0; q < PH; q++) { const double df = row[tt + (h + q) * SVM_T] - xs; r2[q] = fma(df, df, r2[q]); }
        }
#pragma unroll
        for (int q = 0; q < PH; q++) kr[h + q] = fast_exp_neg(gamma * r2[q]);
        SVM_SEQ();
    }
}

// The same row through the row cache: a hit (slot >= 0, hit) reads the thread's own entries of the cached row -- each
// thread reads back only what it stored itself, the same bits it would compute -- a miss computes the row and, given a
// slot, stores it.
template <int PPT, int SVM_T>
__device__ __forceinline__ void svm_row_cached(const double* __restrict__ Xt, int Npad, int dpad, double gamma, int s, int t,
                                               double* cache, int slot, bool hit, double (&kr)[PPT]) {
    double* mine = cache + (size_t)(slot < 0 ? 0 : slot) * Npad + t;
    if (hit) {
#pragma unroll
        for (int q = 0; q < PPT; q++) kr[q] = mine[q * SVM_T];
    } else {
        svm_row<PPT, SVM_T>(Xt, Npad, dpad, gamma, s, t, kr);
        if (slot >= 0) {
#pragma unroll
            for (int q = 0; q < PPT; q++) mine[q * SVM_T] = kr[q];
        }
    }
}

template <int PPT, int SVM_T>
__global__ __launch_bounds__(SVM_T) void svm_smo_kernel(const double* __restrict__ Xt, int Npad, int N, int dpad, double C,
                                                        double gamma, double eps, long long iters,
                                                        double* __restrict__ alpha_g, double* __restrict__ grad_g,
                                                        const signed char* __restrict__ label, SvmStatus* __restrict__ status,
                                                        double* cache, int cache_rows) {
    constexpr int SVM_WAVES = SVM_T / 64;
    __shared__ short slot_of[PPT * SVM_T];      // row -> slot of the row cache (-1: not cached); written by thread 0 only
    __shared__ SvmPart partA[SVM_MAX_WAVES], partB[SVM_MAX_WAVES];
    __shared__ double redS[4][SVM_MAX_WAVES];
    __shared__ int redI[SVM_MAX_WAVES];
    __shared__ SvmCtl ctl;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double a[PPT], g[PPT];
    int y[PPT];                         // +1 finite, -1 infinite, 0 padding
#pragma unroll
    for (int q = 0; q < PPT; q++) {
        const int p = t + q * SVM_T;            // < Npad = PPT * SVM_T: the buffers are padded (label 0: in no index set)
        a[q] = alpha_g[p]; g[q] = grad_g[p]; y[q] = (int)label[p];
        slot_of[p] = -1;                        // the cache starts empty with every launch (a cached row is the computed row, bit for bit)
    }
    // workgroup-uniform bookkeeping of the cache, kept by every thread alike: rows cached so far, and the rows stored in
    // this iteration, whose table entries thread 0 writes between the second and the third barrier (nobody reads then)
    int n_cached = 0, pi_s = -1, pi_slot = -1, pj_s = -1, pj_slot = -1;
    __syncthreads();
    const int fresh_in = status->fresh;
    long long done = 0;
    int state = 0;
    for (;;) {
        // ---- i: argmax of -y G over I_up = {y = +1, alpha < C} U {y = -1, alpha > 0}
        double bv = 0.0; int bi = -1;
#pragma unroll
        for (int q = 0; q < PPT; q++) {
            const bool up = (y[q] > 0 && a[q] < C) || (y[q] < 0 && a[q] > 0.0);
            const double v = -(double)y[q] * g[q];
            if (up && (bi < 0 || v > bv)) { bv = v; bi = t + q * SVM_T; }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const double ov = svm_shfl(bv, m); const int oi = __shfl_xor(bi, m, 64);
            if (svm_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { partA[wave].v = bv; partA[wave].idx = bi; }
        __syncthreads();
        // every wave folds the partials itself (lanes 0 .. waves - 1 take one each; the tie rule makes the order immaterial)
        double gmax = lane < SVM_WAVES ? partA[lane & (SVM_MAX_WAVES - 1)].v : 0.0;
        int i = lane < SVM_WAVES ? partA[lane & (SVM_MAX_WAVES - 1)].idx : -1;
#pragma unroll
        for (int m = 1; m < SVM_WAVES; m <<= 1) {
            const double ov = svm_shfl(gmax, m); const int oi = __shfl_xor(i, m, 64);
            if (svm_better(ov, oi, gmax, i)) { gmax = ov; i = oi; }
        }
        gmax = __shfl(gmax, 0, 64); i = __shfl(i, 0, 64);
        // row i of the kernel for the thread's points (an empty I_up reads row 0 and is stopped by thread 0 below)
        const int iu = __builtin_amdgcn_readfirstlane(i < 0 ? 0 : i);
        double ki[PPT];
        {
            int slot = iu == pj_s ? pj_slot : (int)slot_of[iu];
            const bool hit = slot >= 0;
            pi_s = -1;
            if (!hit && n_cached < cache_rows) { slot = n_cached++; pi_s = iu; pi_slot = slot; }
            svm_row_cached<PPT, SVM_T>(Xt, Npad, dpad, gamma, iu, t, cache, slot, hit, ki);
        }
        // ---- j: argmin of -b^2 / a over I_low = {y = +1, alpha > 0} U {y = -1, alpha < C} with b = G_max + y G > 0;
        //      G_min = min of -y G over I_low (here as its negative, the maximum of y G)
        double jv = 0.0; int jq = -1; double m2 = 0.0; int have2 = 0;
#pragma unroll
        for (int q = 0; q < PPT; q++) {
            const bool low = (y[q] > 0 && a[q] > 0.0) || (y[q] < 0 && a[q] < C);
            const double yg = (double)y[q] * g[q];
            if (low && (!have2 || yg > m2)) { m2 = yg; have2 = 1; }
            const double b = gmax + yg;
            double qd = 2.0 - 2.0 * ki[q];
            if (!(qd > 0.0)) qd = SVM_TAU;
            const double v = (b * b) / qd;                 // maximised: the minimum of its negative
            if (low && b > 0.0 && (jq < 0 || v > jv)) { jv = v; jq = q; }
        }
        int ji = jq < 0 ? -1 : t + jq * SVM_T;
        const int mine = ji;
        double pa = 0.0, pg = 0.0, py = 0.0, pk = 0.0;
#pragma unroll
        for (int q = 0; q < PPT; q++)
            if (q == jq) { pa = a[q]; pg = g[q]; py = (double)y[q]; pk = ki[q]; }
        // the owner of i hands its alpha and gradient on the same way (k_ii is not needed)
        double ia = 0.0, ig = 0.0, iy = 0.0; int iown = 0;
#pragma unroll
        for (int q = 0; q < PPT; q++)
            if (t + q * SVM_T == i) { ia = a[q]; ig = g[q]; iy = (double)y[q]; iown = 1; }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const double ov = svm_shfl(jv, m); const int oi = __shfl_xor(ji, m, 64);
            if (svm_better(ov, oi, jv, ji)) { jv = ov; ji = oi; }
            const double o2 = svm_shfl(m2, m); const int oh = __shfl_xor(have2, m, 64);
            if (oh && (!have2 || o2 > m2)) { m2 = o2; have2 = 1; }
        }
        if (lane == 0) { partB[wave].v = jv; partB[wave].idx = ji; redS[0][wave] = m2; redI[wave] = have2; }
        if (mine >= 0 && mine == ji) {          // the one lane of the wave that holds the wave's best: its payload
            partB[wave].a = pa; partB[wave].g = pg; partB[wave].y = py; partB[wave].k = pk;
        }
        if (iown) { partA[0].a = ia; partA[0].g = ig; partA[0].y = iy; }      // (partA's v / idx were read before this barrier's twin above ...
        __syncthreads();                                                          //  ... and a / g / y are read only behind this one)
        // ---- wave 0 folds the partials, its first thread takes the stop decision and solves the two-variable problem
        //      (libsvm Solver::Solve)
        if (wave == 0) {
            const int ls = lane & (SVM_MAX_WAVES - 1);
            double bvj = lane < SVM_WAVES ? partB[ls].v : 0.0;
            int j = lane < SVM_WAVES ? partB[ls].idx : -1, wj = ls;
            double gmax2 = lane < SVM_WAVES ? redS[0][ls] : 0.0;
            int h2 = lane < SVM_WAVES ? redI[ls] : 0;
#pragma unroll
            for (int m = 1; m < SVM_WAVES; m <<= 1) {
                const double ov = svm_shfl(bvj, m); const int oi = __shfl_xor(j, m, 64), ow = __shfl_xor(wj, m, 64);
                if (svm_better(ov, oi, bvj, j)) { bvj = ov; j = oi; wj = ow; }
                const double o2 = svm_shfl(gmax2, m); const int oh = __shfl_xor(h2, m, 64);
                if (oh && (!h2 || o2 > gmax2)) { gmax2 = o2; h2 = 1; }
            }
          if (lane == 0) {
            if (pi_s >= 0) slot_of[pi_s] = (short)pi_slot;
            if (pj_s >= 0) slot_of[pj_s] = (short)pj_slot;
            SvmCtl c;
            c.i = i; c.j = j; c.slot_j = j < 0 ? -1 : (int)slot_of[j]; c.ai = c.aj = c.ci = c.cj = 0.0;
            c.stop = 0;
            if (i < 0 || j < 0 || !h2 || !(gmax + gmax2 >= eps)) c.stop = 1;         // converged (or nothing left to select)
            else if (done >= iters) c.stop = 2;                                      // the launch's budget
            if (!c.stop) {
                const double yi = partA[0].y, yj = partB[wj].y, kij = partB[wj].k;
                const double Gi = partA[0].g, Gj = partB[wj].g, oai = partA[0].a, oaj = partB[wj].a;
                double ai = oai, aj = oaj;
                const double Qij = yi * yj * kij;
                if (yi != yj) {
                    double quad = 2.0 + 2.0 * Qij;
                    if (!(quad > 0.0)) quad = SVM_TAU;
                    const double delta = (-Gi - Gj) / quad, diff = ai - aj;
                    ai += delta; aj += delta;
                    if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
                    else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
                    if (diff > 0.0) { if (ai > C) { ai = C; aj = C - diff; } }
                    else { if (aj > C) { aj = C; ai = C + diff; } }
                } else {
                    double quad = 2.0 - 2.0 * Qij;
                    if (!(quad > 0.0)) quad = SVM_TAU;
                    const double delta = (Gi - Gj) / quad, sum = ai + aj;
                    ai -= delta; aj += delta;
                    if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
                    else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
                    if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
                    else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
                }
                c.ai = ai; c.aj = aj; c.ci = yi * (ai - oai); c.cj = yj * (aj - oaj);
            }
            redS[1][0] = gmax; redS[1][1] = h2 ? -gmax2 : gmax;
            ctl = c;
          }
        }
        __syncthreads();
        const int stop = ctl.stop;
        if (stop) { state = stop == 1 ? ((fresh_in && done == 0) ? 2 : 1) : 0; break; }
        // ---- the step: G_k += Q_ki d alpha_i + Q_kj d alpha_j with Q_ks = y_k y_s k_ks
        const int j = ctl.j;
        const double nai = ctl.ai, naj = ctl.aj, ci = ctl.ci, cj = ctl.cj;
        const int ju = __builtin_amdgcn_readfirstlane(j);
        double kj[PPT];
        {
            int slot = ctl.slot_j;
            const bool hit = slot >= 0;
            pj_s = -1;
            if (!hit && n_cached < cache_rows) { slot = n_cached++; pj_s = ju; pj_slot = slot; }
            svm_row_cached<PPT, SVM_T>(Xt, Npad, dpad, gamma, ju, t, cache, slot, hit, kj);
        }
#pragma unroll
        for (int q = 0; q < PPT; q++) {
            const double yq = (double)y[q];
            g[q] = fma(yq * kj[q], cj, fma(yq * ki[q], ci, g[q]));
            const int p = t + q * SVM_T;
            if (p == i) a[q] = nai;
            if (p == j) a[q] = naj;
        }
        done++;
    }
    // ---- the state goes back to device memory; objective 1/2 sum alpha (G - 1), rho (libsvm calculate_rho) and the
    //      two ends of the stop test from the same registers (fixed trees: wave, then the 16 partials in order)
    double s_obj = 0.0, s_free = 0.0, ub = INFINITY, lb = -INFINITY; int n_free = 0;
    int te = t;
    asm volatile("" : "+v"(te));     // the addresses are formed again here, not carried through the loop in registers
#pragma unroll
    for (int q = 0; q < PPT; q++) {
        const int p = te + q * SVM_T;
        alpha_g[p] = a[q]; grad_g[p] = g[q];
        if (y[q] != 0) {
            s_obj = fma(a[q], g[q] - 1.0, s_obj);
            const double yg = (double)y[q] * g[q];
            if (a[q] >= C) { if (y[q] < 0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
            else if (a[q] <= 0.0) { if (y[q] > 0) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
            else { n_free++; s_free += yg; }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        s_obj += svm_shfl(s_obj, m); s_free += svm_shfl(s_free, m); n_free += __shfl_xor(n_free, m, 64);
        ub = fmin(ub, svm_shfl(ub, m)); lb = fmax(lb, svm_shfl(lb, m));
    }
    if (lane == 0) { redS[0][wave] = s_obj; redS[2][wave] = s_free; redS[3][wave] = ub; partA[wave].a = lb; redI[wave] = n_free; }
    __syncthreads();
    if (t == 0) {
        double o = 0.0, f = 0.0, u = INFINITY, l = -INFINITY; int nf = 0;
        for (int w = 0; w < SVM_WAVES; w++) {
            o += redS[0][w]; f += redS[2][w]; u = fmin(u, redS[3][w]); l = fmax(l, partA[w].a); nf += redI[w];
        }
        status->n_iter += done;
        status->state = state;
        status->fresh = 0;
        status->rho = nf > 0 ? f / (double)nf : (u + l) / 2.0;
        status->objective = 0.5 * o;
        status->gmax = redS[1][0]; status->gmin = redS[1][1];
    }
}

// G = Q alpha - e from alpha: thread <-> point t, the rows s with alpha_s > 0 in ascending order (s is workgroup-uniform)
__global__ __launch_bounds__(256) void svm_grad_kernel(const double* __restrict__ Xt, int Npad, int N, int dpad, double gamma,
                                                       const double* __restrict__ alpha_g, const signed char* __restrict__ label,
                                                       double* __restrict__ grad_g) {
    const int t = blockIdx.x * 256 + threadIdx.x;         // < Npad (the grid covers Npad exactly)
    double acc = 0.0;
    for (int s = 0; s < N; s++) {
        const double as = alpha_g[s];
        if (!(as > 0.0)) continue;
        double r2 = 0.0;
        for (int k = 0; k < dpad; k++) {
            const double* row = Xt + (size_t)k * Npad;
            const double df = row[t] - row[s];
            r2 = fma(df, df, r2);
        }
        acc = fma((double)label[s] * as, fast_exp_neg(gamma * r2), acc);
    }
    if (t < N) grad_g[t] = (double)label[t] * acc - 1.0;
}

extern "C" {

int gpry_svm_fit(gpry_ctx* ctx, const double* X, const uint8_t* finite, int64_t N, int64_t d, double C, double gamma,
                 double eps, int64_t max_iter, double* alpha, double* rho, double* objective, double* violation,
                 int64_t* n_iter, int* status, double* device_ms) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_svm_fit: ctx is NULL");
    GPRY_TRY(serve_stop(ctx));
    if (!X || !finite || !alpha) return gpry_fail(ctx, -1, "gpry_svm_fit: X, finite and alpha must not be NULL");
    if (N < 2 || N > SVM_MAX_N) return gpry_fail(ctx, -1, "gpry_svm_fit: N = %lld, need 2 <= N <= %d", (long long)N, SVM_MAX_N);
    if (d < 1 || d > GPRY_MAX_DIM) return gpry_fail(ctx, -1, "gpry_svm_fit: d = %lld, need 1 <= d <= %d", (long long)d, GPRY_MAX_DIM);
    if (!(C > 0.0) || !isfinite(C) || !(gamma > 0.0) || !isfinite(gamma) || !(eps > 0.0) || !isfinite(eps))
        return gpry_fail(ctx, -1, "gpry_svm_fit: C, gamma and eps must be positive and finite (got %g, %g, %g)", C, gamma, eps);
    if (max_iter < 0) return gpry_fail(ctx, -1, "gpry_svm_fit: max_iter = %lld < 0", (long long)max_iter);
    int64_t n_pos = 0;
    for (int64_t i = 0; i < N; i++) n_pos += finite[i] ? 1 : 0;
    if (n_pos == 0 || n_pos == N) return gpry_fail(ctx, -1, "gpry_svm_fit: the labels hold one class only");
    for (int64_t e = 0; e < N * d; e++)
        if (!isfinite(X[e])) return gpry_fail(ctx, -1, "gpry_svm_fit: X holds a non-finite value (row %lld)", (long long)(e / d));
    // points per thread x threads: 1024 threads are 4 waves per SIMD and 128 registers each, which holds up to 4 points
    // per thread; 8 points spill there, so above N = 4096 the workgroup has 512 threads (256 registers) with 16 points each
    const int ppt = N <= 1024 ? 1 : N <= 2048 ? 2 : N <= 4096 ? 4 : 16;
    const int Npad = ppt == 16 ? SVM_MAX_N : ppt * 1024, dpad = (int)round_up(d, 4);
    // one upload: coordinates (coordinate-major, zero padding), alpha = 0, G = -1, labels (0 behind N), the status block
    // ... and behind them, not uploaded, the row cache: up to 32 MB of kernel rows (all of them up to N = 2048)
    const int64_t cache_rows = std::min<int64_t>(N, ((int64_t)4 << 20) / Npad);
    const int64_t sz[6] = {8 * (int64_t)dpad * Npad, 8 * (int64_t)Npad, 8 * (int64_t)Npad, (int64_t)Npad, (int64_t)sizeof(SvmStatus),
                           8 * cache_rows * Npad};
    int64_t off[7];
    ns_layout(sz, off);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (off[5] > ctx->hsvm_cap) {            // the image is built in pinned memory of the call's own (a pageable copy above 1 MB pins per call)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->hsvm) HIP_TRY(ctx, hipHostFree(ctx->hsvm));
        ctx->hsvm = nullptr; ctx->hsvm_cap = 0;
        HIP_TRY(ctx, hipHostMalloc(&ctx->hsvm, (size_t)off[5], hipHostMallocDefault));
        ctx->hsvm_cap = off[5];
    }
    uint8_t* host = (uint8_t*)ctx->hsvm;
    memset(host, 0, (size_t)off[5]);
    {
        double* xt = (double*)(host + off[0]);
        double* g0 = (double*)(host + off[2]);
        signed char* lab = (signed char*)(host + off[3]);
        for (int64_t i = 0; i < N; i++) {
            for (int64_t k = 0; k < d; k++) xt[k * Npad + i] = X[i * d + k];
            g0[i] = -1.0;
            lab[i] = finite[i] ? 1 : -1;
        }
    }
    // the call scratch as one region: the device layout is the host image's, offset for offset.  No other claimant is called
    // from here, and everything is queued on ctx->stream, which ns_end drains.
    CallScratch cs(ctx, "gpry_svm_fit");
    const auto rimg = cs.take<uint8_t>(off[6]);
    GPRY_TRY(cs.claim());
    uint8_t* dimg = cs.at(rimg);
    NsTimer tm;
    GPRY_TRY(ns_begin(ctx, &tm));
    hipStream_t st = ctx->stream;
    const double* dXt = (const double*)(dimg + off[0]);
    double *da = (double*)(dimg + off[1]), *dg = (double*)(dimg + off[2]);
    const signed char* dlab = (const signed char*)(dimg + off[3]);
    SvmStatus* dst = (SvmStatus*)(dimg + off[4]);
    double* dcache = (double*)(dimg + off[5]);
    SvmStatus hs;
    memset(&hs, 0, sizeof(hs));
    int result = 1;
    {
        StageScope scope(ctx, "svm_fit");
        HIP_TRY(ctx, hipMemcpyAsync(dimg, host, (size_t)off[5], hipMemcpyHostToDevice, st));
        for (;;) {
            const long long left = (long long)max_iter - hs.n_iter;
            const long long iters = left < (long long)ctx->opt_svm_iters ? left : (long long)ctx->opt_svm_iters;
#define SMO(P, T) hipLaunchKernelGGL((svm_smo_kernel<P, T>), dim3(1), dim3(T), 0, st, dXt, Npad, (int)N, dpad, C, gamma, eps, iters, \
                                     da, dg, dlab, dst, dcache, (int)cache_rows)
            if (ppt == 1) SMO(1, 1024); else if (ppt == 2) SMO(2, 1024); else if (ppt == 4) SMO(4, 1024); else SMO(16, 512);
#undef SMO
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(&hs, dst, sizeof(hs), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (hs.state == 2) { result = 0; break; }
            if (hs.state == 1) {        // the stop test passed on the incremental gradient: repeat it on a recomputed one
                hipLaunchKernelGGL(svm_grad_kernel, dim3((unsigned)(Npad / 256)), dim3(256), 0, st, dXt, Npad, (int)N, dpad, gamma,
                                   da, dlab, dg);
                HIP_TRY(ctx, hipGetLastError());
                hs.fresh = 1;
                HIP_TRY(ctx, hipMemcpyAsync(dst, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
                HIP_TRY(ctx, hipStreamSynchronize(st));       // (hs is written again by the next launch's copy)
                continue;
            }
            if (hs.n_iter >= (long long)max_iter) break;      // the budget: a status, not an error
        }
        HIP_TRY(ctx, hipMemcpyAsync(alpha, da, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    }
    GPRY_TRY(ns_end(ctx, &tm, device_ms));
    if (rho) *rho = hs.rho;
    if (objective) *objective = hs.objective;
    if (violation) *violation = hs.gmax - hs.gmin;
    if (n_iter) *n_iter = (int64_t)hs.n_iter;
    if (status) *status = result;
    return 0;
}

}  // extern "C"
