// Host-only shim around gpry_amd/csrc/kb_rank_core.h for tests/test_kb_rank_cpu.py and kb_rank_selftest.cpp: the ranking
// of gpry_kb_rank with the Gram rows coming from the caller, one row per call of `gram`.
//   speculative >= 0: the rows of the first `speculative` offers in walking order are delivered in front, the rest one
//   request at a time as the core asks; speculative < 0: every row of the session in front.
// Returns the core's value: 0, info = t + 1 > 0, or < 0 on failure.  stats (nullable): rows delivered, requests of the core.
#include <stdint.h>
#include <memory>
#include <vector>
#include "kb_rank_core.h"

extern "C" {
typedef void (*kb_gram_fn)(void* user, int64_t p, double* G, double* kv);

struct HostRows {
    int64_t nn; kb_gram_fn gram; void* user;
    std::vector<const double*> G, kv;
    std::vector<std::unique_ptr<double[]>> store;
    int64_t rows = 0;
    int fetch(const int64_t* p, int n) {
        for (int i = 0; i < n; i++) {
            if (p[i] < 0 || p[i] >= nn) return -2;
            if (G[p[i]]) continue;
            store.emplace_back(new double[(size_t)(2 * nn)]);
            double* blk = store.back().get();
            gram(user, p[i], blk, blk + nn);
            G[p[i]] = blk; kv[p[i]] = blk + nn;
            rows++;
        }
        return 0;
    }
    static int cb(void* u, const int64_t* p, int n) { return static_cast<HostRows*>(u)->fetch(p, n); }
};

int64_t kb_rank_host(int64_t n_session, const double* var0, const int64_t* idx, const double* y, const double* sigma,
                     const double* acq, int64_t n_offer, const int64_t* order, int64_t n_order, const double* params,
                     int64_t n_points, int64_t* slot_idx, double* slot_y, double* slot_sigma, double* slot_acq,
                     double* slot_acq_cond, int64_t* cache_counter, kb_gram_fn gram, void* user, int64_t speculative,
                     int64_t* stats) {
    if (n_session < 1 || n_points < 1 || n_offer < 1 || n_order < 0 || n_order > n_offer) return -2;
    for (int64_t i = 0; i < n_offer; i++) if (idx[i] < 0 || idx[i] >= n_session) return -2;
    for (int64_t k = 0; k < n_order; k++) if (order[k] < 0 || order[k] >= n_offer) return -2;
    HostRows rows{n_session, gram, user};
    rows.G.assign((size_t)n_session, nullptr); rows.kv.assign((size_t)n_session, nullptr);
    if (speculative < 0) {
        for (int64_t p = 0; p < n_session; p++) if (rows.fetch(&p, 1)) return -2;
    } else {
        for (int64_t k = 0; k < n_order && k < speculative; k++) if (rows.fetch(&idx[order[k]], 1)) return -2;
    }
    const int n = (int)n_points;
    kb_rank::Params prm = {params[0], params[1], params[2], params[3], params[4]};
    kb_rank::Pool P = {n, slot_idx, slot_y, slot_sigma, slot_acq, slot_acq_cond, *cache_counter};
    kb_rank::Ranker rk(n, n_session, var0, prm, rows.G.data(), rows.kv.data(), &HostRows::cb, &rows, n_order + n + 1);
    const int64_t rc = rk.add(P, idx, y, sigma, acq, order, n_order);
    *cache_counter = P.cache_counter;
    if (stats) { stats[0] = rows.rows; stats[1] = rk.fetches(); }
    return rc;
}
}
