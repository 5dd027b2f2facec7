// Stand-alone check of gpry_amd/csrc/kb_rank_core.h under the host sanitizers (built with kb_rank_host.cpp; the command
// line is in profiles/multi_add_host.md).  Random U, G = U U^T, kv = G + a positive diagonal excess, random acquisition
// inputs through the core: acq_cond is non-increasing over the filled slots, every index is in range and unique, and the
// result is the same whether the rows are delivered all in front, the first 2 n in front, or one at a time on demand.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

extern "C" {
typedef void (*kb_gram_fn)(void* user, int64_t p, double* G, double* kv);
int64_t kb_rank_host(int64_t n_session, const double* var0, const int64_t* idx, const double* y, const double* sigma,
                     const double* acq, int64_t n_offer, const int64_t* order, int64_t n_order, const double* params,
                     int64_t n_points, int64_t* slot_idx, double* slot_y, double* slot_sigma, double* slot_acq,
                     double* slot_acq_cond, int64_t* cache_counter, kb_gram_fn gram, void* user, int64_t speculative,
                     int64_t* stats);
}

struct Session { int64_t n; int k; std::vector<double> U, kdiag; double C; };

static void gram(void* user, int64_t p, double* G, double* kv) {
    const Session& s = *static_cast<const Session*>(user);
    for (int64_t x = 0; x < s.n; x++) {
        double g = 0.0, r2 = 0.0;
        for (int j = 0; j < s.k; j++) {
            g += s.U[x * s.k + j] * s.U[p * s.k + j];
            const double df = s.U[x * s.k + j] - s.U[p * s.k + j];
            r2 += df * df;
        }
        G[x] = g;
        // a kernel value above the Gram entry, symmetric in (x, p), equal to C on the diagonal
        kv[x] = g + (s.C - 0.5 * (s.kdiag[x] + s.kdiag[p])) * exp(-0.5 * r2);
    }
}

struct Result { std::vector<int64_t> idx; std::vector<double> cond; int64_t counter, info; };

static Result run(const Session& s, int n, const std::vector<double>& var0, const std::vector<double>& y,
                  const std::vector<double>& sd, const std::vector<double>& acq, const std::vector<int64_t>& order,
                  int64_t speculative, int feeds) {
    Result r;
    r.idx.assign(n + 1, -1); r.cond.assign(n + 1, -INFINITY);
    std::vector<double> sy(n + 1, 0.0), ss(n + 1, 0.0), sa(n + 1, 0.0);
    std::vector<int64_t> idx(s.n);
    for (int64_t i = 0; i < s.n; i++) idx[i] = i;
    const double params[5] = {1e-3, 1e-6, 0.0, 0.3, 1.7};
    r.counter = 0; r.info = 0;
    const int64_t per = ((int64_t)order.size() + feeds - 1) / feeds;
    for (int f = 0; f < feeds && r.info == 0; f++) {
        const int64_t o0 = f * per, o1 = std::min<int64_t>((int64_t)order.size(), o0 + per);
        if (o1 <= o0) break;
        r.info = kb_rank_host(s.n, var0.data(), idx.data(), y.data(), sd.data(), acq.data(), s.n, order.data() + o0, o1 - o0,
                              params, n, r.idx.data(), sy.data(), ss.data(), sa.data(), r.cond.data(), &r.counter, gram,
                              const_cast<Session*>(&s), speculative, nullptr);
    }
    return r;
}

int main() {
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> nrm(0.0, 1.0);
    int failures = 0, cases = 0;
    for (int rep = 0; rep < 60; rep++) {
        const int n = 1 + (int)(rng() % 16);
        Session s; s.n = 2 + (int64_t)(rng() % 200); s.k = 1 + (int)(rng() % 6); s.C = 4.0;
        s.U.resize(s.n * s.k); s.kdiag.resize(s.n);
        for (double& u : s.U) u = 0.6 * nrm(rng);
        std::vector<double> var0(s.n), y(s.n), sd(s.n), acq(s.n);
        for (int64_t x = 0; x < s.n; x++) {
            double g = 0.0;
            for (int j = 0; j < s.k; j++) g += s.U[x * s.k + j] * s.U[x * s.k + j];
            if (g > 3.5) { for (int j = 0; j < s.k; j++) s.U[x * s.k + j] *= sqrt(3.5 / g); g = 3.5; }
            s.kdiag[x] = g;
            var0[x] = s.C - g;
            y[x] = nrm(rng); sd[x] = sqrt(var0[x]) * 1.7;
            acq[x] = 0.6 * y[x] + log(sd[x]);
        }
        std::vector<int64_t> order(s.n);
        for (int64_t i = 0; i < s.n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return acq[a] > acq[b]; });
        const Result all = run(s, n, var0, y, sd, acq, order, -1, 1);
        const Result spec = run(s, n, var0, y, sd, acq, order, 2 * n, 1);
        const Result lazy = run(s, n, var0, y, sd, acq, order, 0, 1);
        const Result two = run(s, n, var0, y, sd, acq, order, 0, 2);
        cases++;
        bool ok = all.info >= 0;
        for (const Result* r : {&spec, &lazy, &two})
            ok = ok && r->info == all.info && r->idx == all.idx && r->counter == all.counter &&
                 !memcmp(r->cond.data(), all.cond.data(), sizeof(double) * (n + 1));
        if (all.info == 0) {
            bool open = true;
            for (int t = 0; t < n; t++) {
                if (all.cond[t] == -INFINITY) { open = false; continue; }
                ok = ok && open;                                                   // filled slots are contiguous
                ok = ok && all.idx[t] >= 0 && all.idx[t] < s.n;
                if (t) ok = ok && all.cond[t] <= all.cond[t - 1];
                for (int r = 0; r < t; r++) ok = ok && all.idx[r] != all.idx[t];
            }
            ok = ok && all.cond[n] == -INFINITY;
        }
        if (!ok) { failures++; printf("case %d (n %d, session %lld, info %lld): FAILED\n", rep, n, (long long)s.n, (long long)all.info); }
    }
    printf("kb_rank_selftest: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
