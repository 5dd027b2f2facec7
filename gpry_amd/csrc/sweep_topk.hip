// Shortlist of the resident NORA sweep (gpry_sweep_topk): exact radix select on the 96-bit composite key
// (order-preserving image of acq, candidate index), 12 passes of 8 bits; and the contraction rounds of a pruned sweep.
#include "sweep.h"
#include <algorithm>
#include <functional>

struct SelState { unsigned long long hi; unsigned int lo; unsigned int pad; unsigned long long k_rem; unsigned long long count_ge; };

__device__ __forceinline__ unsigned long long acq_key(double a) {
    unsigned long long b = (unsigned long long)__double_as_longlong(a);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void make_keys_kernel(const double* __restrict__ acq, int64_t M, unsigned long long* __restrict__ keys) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) keys[i] = acq_key(acq[i]);
}
__global__ void exclude_keys_kernel(unsigned long long* keys, const int64_t* excl, int64_t n, int64_t M) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && excl[i] >= 0 && excl[i] < M) keys[excl[i]] = 0ull;   // below key(-inf)
}

// digit of pass p (0 = most significant byte of the acq key ... 7; 8..11 = index bytes)
__device__ __forceinline__ unsigned digit_of(unsigned long long key, unsigned int idx, int pass) {
    return pass < 8 ? (unsigned)((key >> (56 - 8 * pass)) & 0xFF) : (unsigned)((idx >> (24 - 8 * (pass - 8))) & 0xFF);
}
__device__ __forceinline__ bool prefix_match(unsigned long long key, unsigned int idx, const SelState& s, int pass) {
    if (pass == 0) return true;
    if (pass <= 8) {
        int sh = 64 - 8 * pass;
        return sh >= 64 ? true : ((key >> sh) == (s.hi >> sh));
    }
    if (key != s.hi) return false;
    int sh = 32 - 8 * (pass - 8);
    return (idx >> sh) == (s.lo >> sh);
}

__global__ __launch_bounds__(256) void select_hist_kernel(const unsigned long long* __restrict__ keys, int64_t M,
                                                          const SelState* __restrict__ st, int pass,
                                                          unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    SelState s = *st;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < M; i += stride) {
        unsigned long long k = keys[i];
        if (k == 0ull) continue;   // excluded
        if (prefix_match(k, (unsigned)i, s, pass)) atomicAdd(&h[digit_of(k, (unsigned)i, pass)], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
__global__ void select_scan_kernel(unsigned int* hist, SelState* st, int pass) {
    if (threadIdx.x != 0) return;
    SelState s = *st;
    unsigned long long k = s.k_rem, acc = 0;
    int dsel = 0;
    for (int dgt = 255; dgt >= 0; dgt--) {
        unsigned long long c = hist[dgt];
        if (acc + c >= k) { dsel = dgt; break; }
        acc += c;
    }
    s.k_rem = k - acc;
    if (pass < 8) s.hi |= ((unsigned long long)dsel) << (56 - 8 * pass);
    else s.lo |= ((unsigned int)dsel) << (24 - 8 * (pass - 8));
    *st = s;
    for (int dgt = 0; dgt < 256; dgt++) hist[dgt] = 0;
}
// emit every candidate whose composite key >= threshold; track the best one below it
__global__ void select_emit_kernel(const unsigned long long* __restrict__ keys, int64_t M, const SelState* __restrict__ st,
                                   const double* __restrict__ acq, const double* __restrict__ y,
                                   const double* __restrict__ sig, gpry_cand* __restrict__ out, int64_t cap,
                                   unsigned long long* counters /*[0]=n_out, [1]=max key below*/) {
    SelState s = *st;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long best_below = 0ull;
    for (; i < M; i += stride) {
        unsigned long long k = keys[i];
        if (k == 0ull) continue;
        bool ge = (k > s.hi) || (k == s.hi && (unsigned)i >= s.lo);
        if (ge) {
            unsigned long long pos = atomicAdd(&counters[0], 1ull);
            if ((int64_t)pos < cap) { gpry_cand c; c.acq = acq[i]; c.y = y[i]; c.sigma = sig[i]; c.idx = i; out[pos] = c; }
        } else if (k > best_below) best_below = k;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned long long o = __shfl_xor(best_below, off);
        if (o > best_below) best_below = o;
    }
    if ((threadIdx.x & 63) == 0 && best_below) atomicMax(&counters[1], best_below);
}

// ---- option "select_fused": the same 12 passes without the scan launches ----------------------------------------
// Pass p histograms into its own counters hist[p]; the launch of pass p + 1 (and the emit launch for p = 11) first derives
// the digit of pass p from them -- every block for itself: a suffix scan of the 256 counters over 256 threads -- and block 0
// leaves the state in slot p + 1 for the launch after it.  A launch reads slot p and writes slot p + 1: no slot is read and
// written in one launch, and no workgroup waits for another.  One memset per select clears all the counters.

// state after pass `pass`, from the state `s` pass `pass` was histogrammed with and its counters (select_scan_kernel's walk:
// the largest digit whose suffix count reaches k_rem); blockDim.x = 256, every thread returns the same state
__device__ __forceinline__ SelState next_state(SelState s, const unsigned int* __restrict__ hist, int pass) {
    __shared__ unsigned long long suf[2][256 + 1];
    __shared__ unsigned long long pick[2];      // digit, count above it
    const int t = threadIdx.x;
    suf[0][t] = hist[t];
    if (t == 0) { suf[0][256] = 0; suf[1][256] = 0; }
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1) {      // suf[t] = sum of the counters t .. 255
        suf[cur ^ 1][t] = suf[cur][t] + (t + off < 256 ? suf[cur][t + off] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long k = s.k_rem, here = suf[cur][t], above = suf[cur][t + 1];
    if (here >= k && above < k) { pick[0] = (unsigned long long)t; pick[1] = above; }
    if (t == 0 && here < k) { pick[0] = 0ull; pick[1] = here; }         // (fewer keys than k_rem: digit 0, as the walk ends)
    __syncthreads();
    const unsigned long long dsel = pick[0];
    s.k_rem = k - pick[1];
    if (pass < 8) s.hi |= dsel << (56 - 8 * pass);
    else s.lo |= ((unsigned int)dsel) << (24 - 8 * (pass - 8));
    __syncthreads();                            // (the arrays are free again)
    return s;
}
__device__ __forceinline__ SelState first_state(unsigned long long K) {
    SelState s; s.hi = 0ull; s.lo = 0u; s.pad = 0u; s.k_rem = K; s.count_ge = 0ull;
    return s;
}

// hist: this pass's 256 counters (cleared); slots: the 12 states, slot p = the state pass p is histogrammed with
__global__ __launch_bounds__(256) void select_hist_fused_kernel(const unsigned long long* __restrict__ keys, int64_t M,
                                                                unsigned long long K, SelState* __restrict__ slots,
                                                                int pass, unsigned int* __restrict__ hist_all) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    const SelState s = pass == 0 ? first_state(K) : next_state(slots[pass - 1], hist_all + 256 * (pass - 1), pass - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) slots[pass] = s;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < M; base += stride) {      // (uniform over the block)
        const int64_t i = base + threadIdx.x;
        unsigned long long k = i < M ? keys[i] : 0ull;
        const bool act = k != 0ull && prefix_match(k, (unsigned)i, s, pass);       // (0: excluded, or past the end)
        const unsigned dg = act ? digit_of(k, (unsigned)i, pass) : 0u;
        const unsigned long long m = __ballot(act);
        if (m == 0ull) continue;
        // all active lanes on one digit (the leading bytes of a pool of similar values): one add of their number
        const int first = __ffsll((long long)m) - 1;
        const unsigned d0 = (unsigned)__shfl((int)dg, first);
        if (__ballot(act && dg == d0) == m) {
            if (lane == first) atomicAdd(&h[d0], (unsigned)__popcll(m));
        } else if (act) atomicAdd(&h[dg], 1u);
    }
    __syncthreads();
    unsigned int* hist = hist_all + 256 * pass;
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// select_emit_kernel behind the fused passes: the threshold from slot 11 and the counters of pass 11; one atomicMax per block
__global__ __launch_bounds__(256) void select_emit_fused_kernel(const unsigned long long* __restrict__ keys, int64_t M,
                                                                const SelState* __restrict__ slots,
                                                                const unsigned int* __restrict__ hist_all,
                                                                const double* __restrict__ acq, const double* __restrict__ y,
                                                                const double* __restrict__ sig, gpry_cand* __restrict__ out,
                                                                int64_t cap, unsigned long long* counters) {
    __shared__ unsigned long long wbest[4];
    const SelState s = next_state(slots[11], hist_all + 256 * 11, 11);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long best_below = 0ull;
    for (; i < M; i += stride) {
        unsigned long long k = keys[i];
        if (k == 0ull) continue;
        bool ge = (k > s.hi) || (k == s.hi && (unsigned)i >= s.lo);
        if (ge) {
            unsigned long long pos = atomicAdd(&counters[0], 1ull);
            if ((int64_t)pos < cap) { gpry_cand c; c.acq = acq[i]; c.y = y[i]; c.sigma = sig[i]; c.idx = i; out[pos] = c; }
        } else if (k > best_below) best_below = k;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned long long o = __shfl_xor(best_below, off);
        if (o > best_below) best_below = o;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best_below;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) if (wbest[w] > best_below) best_below = wbest[w];
        if (best_below) atomicMax(&counters[1], best_below);
    }
}

// all sweep results as shortlist records (small pools: selected on the host)
__global__ void cand_records_kernel(const double* __restrict__ acq, const double* __restrict__ y, const double* __restrict__ sig,
                                    int64_t M, gpry_cand* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    gpry_cand c;
    c.acq = acq[i]; c.y = y[i]; c.sigma = sig ? sig[i] : 0.0; c.idx = i;
    out[i] = c;
}

// the shortlist's total order (acq desc, idx desc); NaN first as np.argsort(acq)[::-1] would put it
static bool cand_before(const gpry_cand& a, const gpry_cand& b) {
    unsigned long long ka, kb; double x = a.acq, y = b.acq;
    memcpy(&ka, &x, 8); memcpy(&kb, &y, 8);
    ka = (ka >> 63) ? ~ka : (ka | 0x8000000000000000ull);
    kb = (kb >> 63) ? ~kb : (kb | 0x8000000000000000ull);
    if (ka != kb) return ka > kb;
    return a.idx > b.idx;
}
static double key_to_acq(unsigned long long k) {
    unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double a; memcpy(&a, &b, 8); return a;
}

// Exact device top-K of src[0..M) under the composite key (value desc, idx desc; NaN first), exclusions removed: K records
// (acq, y, sigma of the resident sweep, idx) in ctx->dcand, in no particular order; cnt = [records, key of the best one below]
static int device_select(gpry_ctx* ctx, const double* src, int64_t M, int64_t K, const int64_t* exclude, int64_t n_exclude,
                         unsigned long long cnt[2]) {
    hipStream_t st = ctx->stream;
    GPRY_TRY(dev_grow(ctx, &ctx->dkeys, &ctx->keys_cap, round_up(M, 1024)));
    if (!ctx->dhist) { GPRY_TRY(dev_alloc(ctx, &ctx->dhist, 256)); }
    if (!ctx->dsel) GPRY_TRY(dev_alloc(ctx, &ctx->dsel, gpry_ctx::DSEL_WORDS));
    GPRY_TRY(dev_grow(ctx, &ctx->dcand, &ctx->cand_cap, round_up(K, 1024)));
    unsigned nb = (unsigned)((M + 255) / 256);
    hipLaunchKernelGGL(make_keys_kernel, dim3(nb), dim3(256), 0, st, src, M, ctx->dkeys);
    TmpBuf<int64_t> bex;
    int64_t* dex = nullptr;
    if (n_exclude > 0) {
        GPRY_TRY(bex.alloc(ctx, n_exclude));
        dex = bex.p;
        HIP_TRY(ctx, hipMemcpyAsync(dex, exclude, sizeof(int64_t) * n_exclude, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(exclude_keys_kernel, dim3((unsigned)((n_exclude + 255) / 256)), dim3(256), 0, st,
                           ctx->dkeys, dex, n_exclude, M);
    }
    if (K <= 0) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return 0;
    }
    unsigned long long* dcnt = ctx->dsel + gpry_ctx::DSEL_EMIT;
    if (ctx->opt_select_fused) {
        if (!ctx->dselp) GPRY_TRY(dev_alloc(ctx, &ctx->dselp, gpry_ctx::SELP_WORDS));
        SelState* slots = reinterpret_cast<SelState*>(ctx->dselp + gpry_ctx::SELP_HIST_WORDS);      // 12 x 32 bytes
        HIP_TRY(ctx, hipMemsetAsync(dcnt, 0, 16, st));
        HIP_TRY(ctx, hipMemsetAsync(ctx->dselp, 0, sizeof(unsigned int) * gpry_ctx::SELP_HIST_WORDS, st));
        const unsigned nbh = nb < 2048 ? nb : 2048, nbe = nb < 1024 ? nb : 1024;
        for (int pass = 0; pass < 12; pass++)
            hipLaunchKernelGGL(select_hist_fused_kernel, dim3(nbh), dim3(256), 0, st, ctx->dkeys, M, (unsigned long long)K, slots,
                               pass, ctx->dselp);
        hipLaunchKernelGGL(select_emit_fused_kernel, dim3(nbe), dim3(256), 0, st, ctx->dkeys, M, slots, ctx->dselp, ctx->dacq_all,
                           ctx->dy_all, ctx->dsig_all, ctx->dcand, K, dcnt);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(cnt, dcnt, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if ((int64_t)cnt[0] != K)
            return gpry_fail(ctx, -4, "topk: selected %llu candidates, expected %lld", cnt[0], (long long)K);
        return 0;
    }
    SelState s0; memset(&s0, 0, sizeof(s0)); s0.k_rem = (unsigned long long)K;
    SelState* dst = reinterpret_cast<SelState*>(ctx->dsel + gpry_ctx::DSEL_STATE);      // 32 bytes
    HIP_TRY(ctx, hipMemcpyAsync(dst, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(dcnt, 0, 16, st));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dhist, 0, 256 * sizeof(unsigned int), st));
    unsigned nbs = nb < 2048 ? nb : 2048;
    for (int pass = 0; pass < 12; pass++) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(nbs), dim3(256), 0, st, ctx->dkeys, M, dst, pass, ctx->dhist);
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(64), 0, st, ctx->dhist, dst, pass);
    }
    hipLaunchKernelGGL(select_emit_kernel, dim3(nbs), dim3(256), 0, st, ctx->dkeys, M, dst, ctx->dacq_all,
                       ctx->dy_all, ctx->dsig_all, ctx->dcand, K, dcnt);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(cnt, dcnt, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((int64_t)cnt[0] != K)
        return gpry_fail(ctx, -4, "topk: selected %llu candidates, expected %lld", cnt[0], (long long)K);
    return 0;
}

// the shortlist of the resident acq_all as it stands
static int sweep_topk_plain(gpry_ctx* ctx, int64_t Kp, const int64_t* exclude, int64_t n_exclude,
                            gpry_cand* top, int64_t* n_out, double* bound) {
    const int64_t M = ctx->sw_M;
    if (M <= 0 || !ctx->dacq_all) return gpry_fail(ctx, -1, "topk: no sweep results resident");
    if (M > 0xFFFFFFFFll) return gpry_fail(ctx, -1, "topk: M too large");
    StageScope scope(ctx, "topk");
    hipStream_t st = ctx->stream;
    if (M <= ctx->opt_topk_host) {
        // Small pools (the first iterations of a run: a few thousand candidates): the radix select is 28 dependent
        // launches (0.22 ms whatever M is); one kernel writes all M records into the pinned, device-mapped staging
        // buffer and the host selects -- same total order (acq desc, idx desc; NaN first), same bound.
        GPRY_TRY(ensure_pinned(ctx, (int64_t)sizeof(gpry_cand) * M));
        gpry_cand* hrec = static_cast<gpry_cand*>(ctx->hpin);
        hipLaunchKernelGGL(cand_records_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, ctx->dacq_all,
                           ctx->dy_all, ctx->dsig_all, M, static_cast<gpry_cand*>(ctx->hpin_dev));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(st));
        std::vector<int64_t> ex;
        for (int64_t e = 0; e < n_exclude; e++) if (exclude[e] >= 0 && exclude[e] < M) ex.push_back(exclude[e]);
        std::sort(ex.begin(), ex.end());
        ex.erase(std::unique(ex.begin(), ex.end()), ex.end());
        std::vector<gpry_cand> v;
        v.reserve((size_t)M);
        size_t xi = 0;
        for (int64_t i = 0; i < M; i++) {
            if (xi < ex.size() && ex[xi] == i) { xi++; continue; }
            v.push_back(hrec[i]);
        }
        // the device path counts the exclusions as given (n_valid = M - n_exclude)
        int64_t n_valid = M - (n_exclude > 0 ? n_exclude : 0);
        if (n_valid < 0) n_valid = 0;
        if (n_valid > (int64_t)v.size()) n_valid = (int64_t)v.size();
        const int64_t K = Kp < n_valid ? Kp : n_valid;
        *n_out = 0; *bound = -INFINITY;
        if (K <= 0) return 0;
        const int64_t take = std::min<int64_t>(K + 1, (int64_t)v.size());
        std::partial_sort(v.begin(), v.begin() + take, v.end(), cand_before);
        for (int64_t k = 0; k < K; k++) top[k] = v[(size_t)k];
        *n_out = K;
        if ((int64_t)v.size() > K) *bound = v[(size_t)K].acq;
        return 0;
    }
    int64_t n_valid = M - (n_exclude > 0 ? n_exclude : 0);
    if (n_valid < 0) n_valid = 0;
    int64_t K = Kp < n_valid ? Kp : n_valid;
    *n_out = 0; *bound = -INFINITY;
    unsigned long long cnt[2] = {0, 0};
    GPRY_TRY(device_select(ctx, ctx->dacq_all, M, K, exclude, n_exclude, cnt));
    if (K <= 0) return 0;
    HIP_TRY(ctx, hipMemcpy(top, ctx->dcand, sizeof(gpry_cand) * K, hipMemcpyDeviceToHost));
    std::sort(top, top + K, cand_before);
    *n_out = K;
    *bound = cnt[1] ? key_to_acq(cnt[1]) : -INFINITY;
    return 0;
}

// ------------------------------------------------------------------------------------
// Pruned sweep (option "sweep_prune").  Stage A (gpry_sweep_logexp, run_sweep SWEEP_STAGE_A) left y, the bound ub of every
// candidate's acquisition (sweep_mean_kernel) and acq_all = ub, sig_all = PRUNED_SIGMA.  gpry_sweep_topk then contracts the
// top K' candidates by ub exactly (prune_eval: acq_all, sig_all overwritten with the full sweep's values) and selects on the
// MIXED array, exact values where evaluated and bounds elsewhere.  Since a bound is >= the candidate's exact acquisition,
// its composite key (acq, idx) only moves up: if the K best records of the mixed array are all exact, every candidate of the
// full sweep's top K is among them (a pruned one would sit above the K-th record there too), they come out in the full
// sweep's order, and the value behind them -- max(next exact value, largest bound of a pruned candidate) -- is >= the full
// sweep's bound.  Otherwise the candidates whose bound is not below the K-th exact value found so far are contracted
// (prune_survivors), then K' grows x 8; once it would cover a quarter of the pool the full sweep runs (prune_complete).
// (Why a compact batch gives every candidate the bits of the full sweep: sweep.hip, at prune_eval.)

__global__ void gather_acq_kernel(const double* __restrict__ acq, const int64_t* __restrict__ gidx, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = acq[gidx[i]];
}
__global__ void count_not_below_kernel(const double* __restrict__ a, int64_t n, double tau, unsigned long long* out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (; i < n; i += stride) c += !(a[i] < tau) ? 1ull : 0ull;      // (NaN counts: it would sort first)
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// the pool indices of the selected records not contracted yet (order immaterial: a candidate's bits do not depend on it)
__global__ void cand_idx_kernel(const gpry_cand* __restrict__ c, int64_t n, int64_t* __restrict__ idx, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && c[i].sigma == PRUNED_SIGMA) idx[atomicAdd(cnt, 1ull)] = c[i].idx;
}

// the records (acq, y, sigma, idx) of the selected candidates as the resident arrays hold them now
__global__ void cand_refresh_kernel(const gpry_cand* __restrict__ c, int64_t n, const double* __restrict__ acq,
                                    const double* __restrict__ y, const double* __restrict__ sig, gpry_cand* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t idx = c[i].idx;
    gpry_cand r;
    r.acq = acq[idx]; r.y = y[idx]; r.sigma = sig[idx]; r.idx = idx;
    out[i] = r;
}
static unsigned long long acq_key_host(double a) {
    unsigned long long b; memcpy(&b, &a, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// Option "prune_one_select", for the FIRST round after stage A alone (nothing outside the selected set is contracted): the
// nsel selected records are now exact, every other candidate that counts still holds its bound, and the largest of those
// bound keys is `below` (cnt[1] of the select).  If the Kp-th best exact record lies strictly above it, the Kp best records
// of the mixed array are the Kp best of these nsel, and the value behind them is the larger of record Kp + 1 and that bound:
// what sweep_topk_plain would select from all M values.  *done = 0 in every other case (a tie with the outside bound, too few
// records, a NaN, a record that was not contracted): the caller goes on as without the option.
static int prune_first_round_answer(gpry_ctx* ctx, int64_t Kp, int64_t n_exclude, int64_t nsel, unsigned long long below,
                                    gpry_cand* top, int64_t* n_out, double* bound, int* done) {
    *done = 0;
    const int64_t n_valid = ctx->sw_M - (n_exclude > 0 ? n_exclude : 0);
    if (Kp <= 0 || Kp > nsel || Kp > n_valid) return 0;
    gpry_cand* rec = nullptr;
    {
        StageScope s(ctx, "sweep_prune_select");
        GPRY_TRY(ensure_pinned(ctx, (int64_t)sizeof(gpry_cand) * nsel));
        rec = static_cast<gpry_cand*>(ctx->hpin);
        hipLaunchKernelGGL(cand_refresh_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dcand, nsel,
                           ctx->dacq_all, ctx->dy_all, ctx->dsig_all, static_cast<gpry_cand*>(ctx->hpin_dev));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int64_t i = 0; i < nsel; i++) if (rec[i].acq != rec[i].acq) return 0;
    std::sort(rec, rec + nsel, cand_before);
    for (int64_t i = 0; i < Kp; i++) if (rec[i].sigma == PRUNED_SIGMA) return 0;
    if (!(acq_key_host(rec[Kp - 1].acq) > below)) return 0;
    for (int64_t i = 0; i < Kp; i++) top[i] = rec[i];
    *n_out = Kp;
    unsigned long long kb = below;
    if (nsel > Kp && acq_key_host(rec[Kp].acq) > kb) kb = acq_key_host(rec[Kp].acq);
    *bound = kb ? key_to_acq(kb) : -INFINITY;
    *done = 1;
    return 0;
}

// The survivors of the contracted set (the n_gidx candidates in ctx->dgidx): tau = the Kp-th best exact acquisition among
// them outside the exclusions -- a lower bound of the full sweep's Kp-th value -- and *n_surv = the number of candidates whose
// bound is not below tau; every other candidate is out.  *n_surv = -1 if fewer than Kp of them count.
static int prune_survivors(gpry_ctx* ctx, int64_t Kp, const int64_t* exclude, int64_t n_exclude, int64_t* n_surv) {
    const int64_t n = ctx->prune.n_gidx;
    *n_surv = -1;
    if (n < Kp || Kp <= 0) return 0;
    std::vector<double> a((size_t)n);
    std::vector<int64_t> idx((size_t)n);
    {
        StageScope s(ctx, "sweep_prune_select");
        TmpBuf<double> buf;
        GPRY_TRY(buf.alloc(ctx, n));
        hipLaunchKernelGGL(gather_acq_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dacq_all, ctx->dgidx, n, buf.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(a.data(), buf.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(idx.data(), ctx->dgidx, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::vector<int64_t> ex(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    std::sort(ex.begin(), ex.end());
    std::vector<double> v;
    v.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (a[(size_t)i] != a[(size_t)i]) return 0;                     // NaN: leave it to the full sweep
        if (!std::binary_search(ex.begin(), ex.end(), idx[(size_t)i])) v.push_back(a[(size_t)i]);
    }
    if ((int64_t)v.size() < Kp) return 0;
    std::nth_element(v.begin(), v.begin() + (Kp - 1), v.end(), std::greater<double>());
    const double tau = v[(size_t)(Kp - 1)];
    HIP_TRY(ctx, hipMemsetAsync(ctx->dsel + gpry_ctx::DSEL_SURV, 0, 8, ctx->stream));
    hipLaunchKernelGGL(count_not_below_kernel, dim3(1024), dim3(256), 0, ctx->stream, ctx->dub, ctx->sw_M, tau, ctx->dsel + gpry_ctx::DSEL_SURV);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long c = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&c, ctx->dsel + gpry_ctx::DSEL_SURV, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->prune.tau = tau;
    ctx->prune.survivors = (int64_t)c;
    *n_surv = (int64_t)c;
    return 0;
}

static int prune_topk(gpry_ctx* ctx, int64_t Kp, const int64_t* exclude, int64_t n_exclude,
                      gpry_cand* top, int64_t* n_out, double* bound) {
    const int64_t M = ctx->sw_M;
    ctx->prune.last_K = Kp;
    bool first_round = ctx->opt_prune_one_select && ctx->prune.rounds == 0 && ctx->prune.n_eval == 0;
    for (;;) {
        if (ctx->prune.n_eval > 0) {
            GPRY_TRY(sweep_topk_plain(ctx, Kp, exclude, n_exclude, top, n_out, bound));
            bool exact = true;
            for (int64_t i = 0; i < *n_out && exact; i++) exact = !(top[i].sigma == PRUNED_SIGMA);
            if (exact) return 0;
        }
        // round 1: the top max(4 Kp, 1024) by bound (the threshold stage); round 2: exactly the candidates whose bound is not
        // below the threshold tau that round 1 found (the survivors); after that the set grows x 8
        int64_t kq = Kp > 0 ? 4 * Kp : 1;
        if (kq < 1024) kq = 1024;
        if (ctx->prune.n_eval > 0) {
            int64_t ns = -1;
            if (!ctx->prune.tau_done) {
                ctx->prune.tau_done = 1;
                GPRY_TRY(prune_survivors(ctx, Kp, exclude, n_exclude, &ns));
            }
            if (ns > ctx->prune.n_eval) kq = ns;
            else if (kq < 8 * ctx->prune.n_eval) kq = 8 * ctx->prune.n_eval;
        }
        if (kq > M / 4 || kq > M - (n_exclude > 0 ? n_exclude : 0)) {      // (cheaper, or no longer possible: the full sweep)
            GPRY_TRY(prune_complete(ctx));
            return sweep_topk_plain(ctx, Kp, exclude, n_exclude, top, n_out, bound);
        }
        unsigned long long cnt[2] = {0, 0};
        {
            StageScope s(ctx, "sweep_prune_select");
            GPRY_TRY(device_select(ctx, ctx->dub, M, kq, exclude, n_exclude, cnt));
        }
        const int64_t nsel = (int64_t)cnt[0];
        GPRY_TRY(dev_grow(ctx, &ctx->dgidx, &ctx->gidx_cap, round_up(nsel, 1024)));
        unsigned long long nn = 0;
        if (nsel > 0) {         // (the candidates an earlier round contracted are not contracted again)
            HIP_TRY(ctx, hipMemsetAsync(ctx->dsel + gpry_ctx::DSEL_GIDX, 0, 8, ctx->stream));
            hipLaunchKernelGGL(cand_idx_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dcand, nsel,
                               ctx->dgidx, ctx->dsel + gpry_ctx::DSEL_GIDX);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(&nn, ctx->dsel + gpry_ctx::DSEL_GIDX, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        const int64_t n = (int64_t)nn;
        if (n > 0) GPRY_TRY(prune_eval(ctx, n));
        ctx->prune.n_eval = kq;
        ctx->prune.n_gidx = n;
        ctx->prune.rounds++;
        ctx->prune.evaluated_total += n;
        if (first_round) {
            first_round = false;
            int done = 0;
            GPRY_TRY(prune_first_round_answer(ctx, Kp, n_exclude, nsel, cnt[1], top, n_out, bound, &done));
            if (done) return 0;
        }
    }
}

extern "C" int gpry_sweep_topk(gpry_ctx* ctx, int64_t Kp, const int64_t* exclude, int64_t n_exclude,
                               gpry_cand* top, int64_t* n_out, double* bound) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_topk: ctx is NULL");
    if (!top || !n_out || !bound) return gpry_fail(ctx, -1, "topk: top, n_out and bound must not be NULL");
    if (n_exclude > 0 && !exclude) return gpry_fail(ctx, -1, "topk: n_exclude > 0 but exclude is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->sw_pruned && ctx->sw_M > 0) return prune_topk(ctx, Kp, exclude, n_exclude, top, n_out, bound);
    return sweep_topk_plain(ctx, Kp, exclude, n_exclude, top, n_out, bound);
}

extern "C" int gpry_sweep_prune_info(gpry_ctx* ctx, int64_t* info, double* dinfo) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_prune_info: ctx is NULL");
    if (!info) return gpry_fail(ctx, -1, "sweep_prune_info: info must not be NULL");
    info[0] = ctx->sw_pruned;
    info[1] = ctx->sw_M;
    info[2] = ctx->prune.n_eval;
    info[3] = ctx->prune.rounds;
    info[4] = ctx->prune.evaluated_total;
    info[5] = ctx->prune.completed;
    info[6] = ctx->prune.last_K;
    info[7] = ctx->prune.survivors;
    info[8] = ctx->prune.ybound;
    info[9] = ctx->prune.live_blocks;
    info[10] = ctx->prune.blocks;
    if (dinfo) {
        dinfo[0] = ctx->prune.survivors >= 0 ? ctx->prune.tau : NAN;
        const char* names[] = {"sweep_mean", "sweep_prune_select", "sweep_compact", "sweep_prune_gemm"};
        for (int k = 0; k < 4; k++) {
            double ms = 0.0; int64_t cnt = 0;
            if (gpry_timing_get(ctx, names[k], &ms, &cnt) != 0) ms = 0.0;
            dinfo[1 + k] = ms;
        }
    }
    return 0;
}

extern "C" int gpry_sweep_screen_info(gpry_ctx* ctx, int64_t out[2]) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_sweep_screen_info: ctx is NULL");
    if (!out) return gpry_fail(ctx, -1, "sweep_screen_info: out must not be NULL");
    out[0] = ctx->prune.cert_blocks;
    out[1] = ctx->prune.blocks;
    return 0;
}
