// The Kriging-believer ranking of an offer (gpry_amd/gp_acquisition.py: RankedPool.add "single sort acq", add_one,
// _position_for, sort, cache_model; gpry_amd/kriging.py: ConditionedGPR), on session indices, in plain C++17: no HIP, and no
// allocation once a Ranker is built.  gpry_kb_rank (kb_rank.hip) serves its Gram rows from the device; the host-only shim
// tests/c_abi/kb_rank_host.cpp serves them from the caller.
//
// A pool has n slots and one spare; slot i holds the candidate whose acquisition, evaluated with the standard deviation of
// the model augmented by slots 0..i-1, is the largest among the rest.  The model augmented by the first T slots is a
// bordered factor: row t has c[t][r] (r < t) and the diagonal l[t]; candidate x has the weights w[t] (t < T).
//
// ORDER OF OPERATIONS (what makes the picks those of the Python path; every product is rounded on its own, never fused
// into the sum that takes it -- mul()):
//   border row t, p = slot t, (G, kv) = Gram row of p, for r = 0..t-1 with q = slot r:
//       dot = 0; for j = 0..r-1: dot += c[t][j] * c[r][j]          (index order; numpy's dot sums in BLAS order: the one
//       c[t][r] = ((kv[q] - G[q]) - dot) / l[r]                      place where the two paths may round differently)
//       acc += c[t][r] * c[t][r]                                     (acc from 0.0, r ascending)
//       l2 = ((kv[p] + alpha) - G[p]) - acc;   not l2 > 0: info = t + 1;   l[t] = sqrt(l2)
//   weights of x, t ascending: dot = 0; for r = 0..t-1: dot += c[t][r] * w[r];   w[t] = ((kv[x] - G[x]) - dot) / l[t]
//   std of x under T slots: ss = 0; for t = 0..T-1: ss += w[t] * w[t];  var = var0[x] - ss;  var < 0: 0;  sqrt(var) * y_std
//   acquisition: logexp_value (acq_math.h), the function the device sweep compiles
//   sort: candidates of slots slot..end-1 by min(value, ceiling), descending; equal values keep their slot order
// Rows, border rows and weights are functions of the slot order alone, so they are kept while the slots in front of them
// stay and recomputed behind the first slot that changed -- the values ConditionedGPR's prefix re-use copies.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>
#include "acq_math.h"

namespace kb_rank {

// Deliver the Gram rows of the n session indices p[] into the tables the Ranker was given (G[p], kv[p]; more rows than
// asked for may be delivered).  Non-zero: failure, handed through as the ranking's return value.
typedef int (*fetch_fn)(void* user, const int64_t* p, int n);

struct Params { double sigma_n, alpha, baseline, zeta, y_std; };

// The pool's arrays, n + 1 entries each; idx = session index of the slot's candidate (-1: never filled).
struct Pool {
    int n;
    int64_t* idx; double* y; double* sigma; double* acq; double* acq_cond;
    int64_t cache_counter;
};

static inline double mul(double a, double b) { double p = a * b; GPRY_ACQ_PIN(p); return p; }

class Ranker {
public:
    // G, kv: tables of n_session row pointers (NULL: not delivered yet), filled by fetch.  max_touched: how many distinct
    // candidates may be looked at (offers walked + slots).
    Ranker(int n, int64_t n_session, const double* var0, const Params& prm, const double* const* G, const double* const* kv,
           fetch_fn fetch, void* user, int64_t max_touched)
        : n_(n), ns_(n_session), var0_(var0), prm_(prm), G_(G), kv_(kv), fetch_(fetch), user_(user) {
        c_.assign((size_t)(n + 1) * (n + 1), 0.0);
        l_.assign((size_t)n + 1, 0.0);
        wslot_.assign((size_t)n_session, -1);
        w_.assign((size_t)max_touched * (n + 1), 0.0);
        whave_.assign((size_t)max_touched, 0);
        a_.assign((size_t)n + 1, 0.0);
        rank_.assign((size_t)n + 1, 0);
        tmp_i_.assign((size_t)n + 1, 0);
        tmp_d_.assign((size_t)n + 1, 0.0);
        want_.assign((size_t)n + 1, 0);
        max_touched_ = max_touched;
    }
    int64_t fetches() const { return fetches_; }

    // RankedPool.add: walk the offers in `order`.  Returns 0, the fetch's failure code (< 0), or info = t + 1 > 0 when the
    // t-th appended point makes the bordered matrix non positive definite.
    int64_t add(Pool& P, const int64_t* idx, const double* y, const double* sigma, const double* acq, const int64_t* order,
                int64_t n_order) {
        for (int64_t k = 0; k < n_order; k++) {
            const int64_t i = order[k];
            if (acq[i] <= P.acq_cond[n_ - 1]) break;       // descending acquisition: the rest returns at add_one's first test
            const int64_t rc = add_one(P, idx[i], y[i], sigma[i], acq[i]);
            if (rc) return rc;
        }
        return 0;
    }

private:
    double* c(int t) { return &c_[(size_t)t * (n_ + 1)]; }

    // rows of the slots' candidates that are not here yet, in one request
    int64_t fetch_slots(const Pool& P, int upto) {
        int m = 0;
        for (int t = 0; t <= n_; t++) {
            if (P.idx[t] < 0 || (t >= upto && !(P.acq_cond[t] > -INFINITY))) continue;
            if (!G_[P.idx[t]]) {
                bool dup = false;
                for (int j = 0; j < m; j++) dup = dup || want_[j] == P.idx[t];
                if (!dup) want_[m++] = P.idx[t];
            }
        }
        if (!m) return 0;
        fetches_++;
        return fetch_(user_, want_.data(), m);
    }
    // border rows nvalid_..T-1 (ConditionedGPR.__init__)
    int64_t ensure_factor(const Pool& P, int T) {
        for (int t = nvalid_; t < T; t++) {
            const int64_t p = P.idx[t];
            if (p < 0 || p >= ns_) return -1;
            if (!G_[p]) { const int64_t rc = fetch_slots(P, T); if (rc) return rc < 0 ? rc : -1; }
            if (!G_[p]) return -1;
            const double *G = G_[p], *kv = kv_[p];
            double* ct = c(t);
            double acc = 0.0;
            for (int r = 0; r < t; r++) {
                const int64_t q = P.idx[r];
                const double* cr = c(r);
                double dot = 0.0;
                for (int j = 0; j < r; j++) dot += mul(ct[j], cr[j]);
                const double v = ((kv[q] - G[q]) - dot) / l_[r];
                ct[r] = v;
                acc += mul(v, v);
            }
            const double l2 = ((kv[p] + prm_.alpha) - G[p]) - acc;
            if (!(l2 > 0.0)) return t + 1;
            l_[t] = sqrt(l2);
            nvalid_ = t + 1;
        }
        return 0;
    }
    // the slots from `pos` on changed: what was derived from them goes
    void invalidate(int pos) {
        if (nvalid_ > pos) nvalid_ = pos;
        for (int64_t k = 0; k < ntouched_; k++) if (whave_[k] > pos) whave_[k] = pos;
    }
    // ConditionedGPR.predict_std of the model of the first T slots at candidate x
    int64_t predict_std(const Pool& P, int T, int64_t x, double* out) {
        const int64_t rc = ensure_factor(P, T);
        if (rc) return rc;
        int64_t k = wslot_[x];
        if (k < 0) {
            if (ntouched_ >= max_touched_) return -1;
            k = wslot_[x] = ntouched_++;
            whave_[k] = 0;
        }
        double* w = &w_[(size_t)k * (n_ + 1)];
        for (int t = whave_[k]; t < T; t++) {
            const int64_t p = P.idx[t];
            const double* ct = c(t);
            double dot = 0.0;
            for (int r = 0; r < t; r++) dot += mul(ct[r], w[r]);
            w[t] = ((kv_[p][x] - G_[p][x]) - dot) / l_[t];
        }
        if (whave_[k] < T) whave_[k] = T;
        double ss = 0.0;
        for (int t = 0; t < T; t++) ss += mul(w[t], w[t]);
        double var = var0_[x] - ss;
        if (var < 0.0) var = 0.0;
        *out = sqrt(var) * prm_.y_std;
        return 0;
    }
    double acq_value(double y, double sd) const { return logexp_value(y, sd, prm_.zeta, prm_.baseline, prm_.sigma_n); }

    // first slot, scanning upwards from the bottom, whose conditioned value is >= a_cond decides the provisional rank
    int position_for(const Pool& P, double a_cond) const {
        for (int up = 0; up < n_; up++) if (P.acq_cond[n_ - 1 - up] >= a_cond) return n_ - up;
        return 0;
    }

    int64_t add_one(Pool& P, int64_t x, double y, double sigma, double acq) {
        if (acq <= P.acq_cond[n_ - 1]) return 0;
        double a_cond = acq;
        int last_pos = n_, pos;
        for (;;) {
            pos = position_for(P, a_cond);
            if (pos == 0 || pos == last_pos || pos == n_) break;
            double s_cond;
            const int64_t rc = predict_std(P, pos, x, &s_cond);
            if (rc) return rc;
            const double v = acq_value(y, s_cond);
            if (v < a_cond) a_cond = v;                     // conditioning cannot raise it
            last_pos = pos;
        }
        if (pos >= n_) return 0;
        for (int j = n_; j > pos; j--) {
            P.idx[j] = P.idx[j - 1]; P.y[j] = P.y[j - 1]; P.sigma[j] = P.sigma[j - 1]; P.acq[j] = P.acq[j - 1];
            P.acq_cond[j] = P.acq_cond[j - 1];
        }
        P.idx[pos] = x; P.y[pos] = y; P.sigma[pos] = sigma; P.acq[pos] = acq; P.acq_cond[pos] = a_cond;
        invalidate(pos);
        const int64_t rc = sort(P, pos + 1);
        if (rc) return rc;
        P.acq_cond[n_] = -INFINITY;
        return 0;
    }

    // re-rank slots i_start.. given that the ones above are final (i_start >= 1: add_one never re-ranks slot 0)
    int64_t sort(Pool& P, int i_start) {
        for (int slot = i_start; slot < n_; slot++) {
            const int64_t rc = ensure_factor(P, slot);      // cache_model(slot - 1)
            if (rc) return rc;
            P.cache_counter++;
            if (!(P.acq_cond[slot] > -INFINITY)) return 0;
            int end = n_ + 1;
            for (int j = 0; j <= n_; j++) if (P.acq_cond[j] == -INFINITY) { end = j; break; }
            if (end <= slot) return 0;
            const double ceiling = P.acq_cond[slot - 1];
            const int m = end - slot;
            for (int j = 0; j < m; j++) {
                double s_cond;
                const int64_t rc2 = predict_std(P, slot, P.idx[slot + j], &s_cond);
                if (rc2) return rc2;
                const double v = acq_value(P.y[slot + j], s_cond);
                a_[j] = v < ceiling ? v : ceiling;
                rank_[j] = j;
            }
            // insertion sort, descending, equal values in slot order
            for (int j = 1; j < m; j++) {
                const int rj = rank_[j];
                int k = j;
                while (k > 0 && a_[rank_[k - 1]] < a_[rj]) { rank_[k] = rank_[k - 1]; k--; }
                rank_[k] = rj;
            }
            if (a_[rank_[0]] == -INFINITY) {
                for (int j = slot; j < end; j++) P.acq_cond[j] = -INFINITY;
                return 0;
            }
            int first_change = -1;
            for (int j = 0; j < m; j++) if (rank_[j] != j) { first_change = j; break; }
            if (first_change >= 0) {
                permute(P.idx + slot, m); permute(P.y + slot, m); permute(P.sigma + slot, m); permute(P.acq + slot, m);
                invalidate(slot + first_change);
            }
            for (int j = 0; j < m; j++) P.acq_cond[slot + j] = a_[rank_[j]];
        }
        return 0;
    }
    void permute(int64_t* a, int m) {
        for (int j = 0; j < m; j++) tmp_i_[j] = a[rank_[j]];
        for (int j = 0; j < m; j++) a[j] = tmp_i_[j];
    }
    void permute(double* a, int m) {
        for (int j = 0; j < m; j++) tmp_d_[j] = a[rank_[j]];
        for (int j = 0; j < m; j++) a[j] = tmp_d_[j];
    }

    int n_;
    int64_t ns_;
    const double* var0_;
    Params prm_;
    const double* const* G_;
    const double* const* kv_;
    fetch_fn fetch_;
    void* user_;
    std::vector<double> c_, l_, w_, a_, tmp_d_;
    std::vector<int64_t> wslot_, tmp_i_, want_;
    std::vector<int> whave_, rank_;
    int nvalid_ = 0;
    int64_t ntouched_ = 0, max_touched_ = 0, fetches_ = 0;
};

}  // namespace kb_rank
