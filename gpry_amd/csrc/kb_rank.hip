// gpry_kb_rank: the Kriging-believer ranking of an offer in one library call.  The slot logic is the host's
// (kb_rank_core.h); this file registers the offer (gpry_kb_register: same rows of U, same var0) and serves the core's Gram
// rows from ONE launch per request, grid.y = requested row, per entry the arithmetic of gpry_kb_gram (kb_gram.h).
#include "common.h"
#include "kb_gram.h"
#include "kb_rank_core.h"
#include <memory>

#define KB_ROWS_MAX 64      // rows of one launch (the list travels in the kernel arguments)
struct KbRowList { int64_t p[KB_ROWS_MAX]; };

// row j of the launch, p = rows.p[j]: out[j * 2n + x] = U[x].U[p], out[j * 2n + n + x] = C k(x, p)
__global__ __launch_bounds__(256) void kb_gram_rows_kernel(const double* __restrict__ U, int64_t ldu, int64_t n, KbRowList rows,
                                                           int64_t Np, const double* __restrict__ Xkb, int dpad, int kid,
                                                           double C, double* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n) return;
    double* o = out + (int64_t)blockIdx.y * 2 * n;
    kb_gram_entry(U, ldu, x, rows.p[blockIdx.y], Np, Xkb, dpad, kid, C, o, o + n);
}

namespace {
struct RowServer {
    gpry_ctx* ctx;
    int64_t nn;                                     // registered candidates = length of a row
    std::vector<const double*> G, kv;               // per session index
    std::vector<std::unique_ptr<double[]>> store;   // one block per request
    int64_t launches = 0, rows = 0;

    // Gram rows of p[0..n), those not yet here, through the pinned, mapped buffer
    int fetch(const int64_t* p, int n) {
        std::vector<int64_t> want;
        for (int i = 0; i < n; i++) {
            if (p[i] < 0 || p[i] >= nn) return gpry_fail(ctx, -1, "kb_rank: index %lld out of range [0, %lld)", (long long)p[i], (long long)nn);
            bool have = G[p[i]] != nullptr;
            for (int64_t w : want) have = have || w == p[i];
            if (!have) want.push_back(p[i]);
        }
        for (size_t b0 = 0; b0 < want.size(); b0 += KB_ROWS_MAX) {
            const int cnt = (int)std::min<size_t>(KB_ROWS_MAX, want.size() - b0);
            KbRowList rl = {};
            for (int j = 0; j < cnt; j++) rl.p[j] = want[b0 + j];
            const int64_t len = 2 * nn * cnt;
            GPRY_TRY(ensure_pinned(ctx, (int64_t)sizeof(double) * len));
            hipLaunchKernelGGL(kb_gram_rows_kernel, dim3((unsigned)((nn + 3) / 4), (unsigned)cnt), dim3(256), 0, ctx->stream,
                               ctx->dU, ctx->Np, nn, rl, ctx->Np, ctx->dXkb, ctx->dpad, ctx->kernel_id, exp(ctx->theta[0]),
                               static_cast<double*>(ctx->hpin_dev));
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            store.emplace_back(new double[(size_t)len]);
            double* blk = store.back().get();
            memcpy(blk, ctx->hpin, sizeof(double) * (size_t)len);
            for (int j = 0; j < cnt; j++) { G[rl.p[j]] = blk + (size_t)j * 2 * nn; kv[rl.p[j]] = blk + (size_t)j * 2 * nn + nn; }
            launches++; rows += cnt;
        }
        return 0;
    }
    static int fetch_cb(void* user, const int64_t* p, int n) { return static_cast<RowServer*>(user)->fetch(p, n); }
};
}  // namespace

extern "C" {

int gpry_kb_gram_rows(gpry_ctx* ctx, const int64_t* p, int64_t n_rows, double* G, double* kvec, int64_t* n) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kb_gram_rows: ctx is NULL");
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!p || !G || !kvec || n_rows <= 0 || n_rows > 16384) return gpry_fail(ctx, -1, "kb_gram_rows: bad arguments");
    if (ctx->kb_n <= 0) return gpry_fail(ctx, -1, "kb_gram_rows: no registered candidates");
    StageScope kb_scope(ctx, "kb_rank");
    RowServer rs{ctx, ctx->kb_n};
    rs.G.assign((size_t)rs.nn, nullptr); rs.kv.assign((size_t)rs.nn, nullptr);
    GPRY_TRY(rs.fetch(p, (int)n_rows));
    for (int64_t j = 0; j < n_rows; j++) {
        memcpy(G + j * rs.nn, rs.G[p[j]], sizeof(double) * rs.nn);
        memcpy(kvec + j * rs.nn, rs.kv[p[j]], sizeof(double) * rs.nn);
    }
    if (n) *n = rs.nn;
    return 0;
}

int gpry_kb_rank(gpry_ctx* ctx, const double* X_new, int64_t m_new, double* var0, int64_t n_session,
                 const int64_t* idx, const double* y, const double* sigma, const double* acq, int64_t n_offer,
                 const int64_t* order, int64_t n_order, const double* params, int64_t n_points,
                 int64_t* slot_idx, double* slot_y, double* slot_sigma, double* slot_acq, double* slot_acq_cond,
                 int64_t* cache_counter, int64_t* info, int64_t* stats) {
    if (!ctx) return gpry_fail(nullptr, -1, "gpry_kb_rank: ctx is NULL");
    GPRY_TRY(require_model(ctx, true));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!var0 || !idx || !y || !sigma || !acq || !order || !params || !slot_idx || !slot_y || !slot_sigma || !slot_acq ||
        !slot_acq_cond || !cache_counter || !info)
        return gpry_fail(ctx, -1, "kb_rank: NULL argument");
    if (n_points < 1 || n_points > 4096 || n_offer < 1 || n_offer > 16384 || n_order < 0 || n_order > n_offer || m_new < 0 ||
        (m_new > 0 && !X_new))
        return gpry_fail(ctx, -1, "kb_rank: bad sizes (n_points %lld, offer %lld, order %lld, new rows %lld)", (long long)n_points,
                         (long long)n_offer, (long long)n_order, (long long)m_new);
    *info = 0;
    if (m_new > 0) {
        int64_t first = -1;
        if (ctx->kb_n + m_new != n_session)
            return gpry_fail(ctx, -1, "kb_rank: session has %lld candidates, %lld new rows, caller expects %lld",
                             (long long)ctx->kb_n, (long long)m_new, (long long)n_session);
        GPRY_TRY(gpry_kb_register(ctx, X_new, m_new, &first, var0 + (n_session - m_new)));
    }
    if (ctx->kb_n != n_session)
        return gpry_fail(ctx, -1, "kb_rank: session has %lld candidates, caller expects %lld", (long long)ctx->kb_n, (long long)n_session);
    for (int64_t i = 0; i < n_offer; i++)
        if (idx[i] < 0 || idx[i] >= n_session) return gpry_fail(ctx, -1, "kb_rank: offer %lld has session index %lld", (long long)i, (long long)idx[i]);
    for (int64_t k = 0; k < n_order; k++)
        if (order[k] < 0 || order[k] >= n_offer) return gpry_fail(ctx, -1, "kb_rank: order[%lld] = %lld", (long long)k, (long long)order[k]);
    const int n = (int)n_points;
    for (int t = 0; t <= n; t++)
        if (slot_idx[t] >= n_session || (slot_idx[t] < 0 && slot_acq_cond[t] > -INFINITY))
            return gpry_fail(ctx, -1, "kb_rank: slot %d has session index %lld", t, (long long)slot_idx[t]);
    StageScope kb_scope(ctx, "kb_rank");
    RowServer rs{ctx, n_session};
    rs.G.assign((size_t)n_session, nullptr); rs.kv.assign((size_t)n_session, nullptr);
    {   // the speculative request: the pool's slots and the first 2 n offers in walking order
        std::vector<int64_t> spec;
        for (int t = 0; t < n; t++) if (slot_idx[t] >= 0 && slot_acq_cond[t] > -INFINITY) spec.push_back(slot_idx[t]);
        for (int64_t k = 0; k < n_order && k < 2 * (int64_t)n; k++) spec.push_back(idx[order[k]]);
        if (!spec.empty()) GPRY_TRY(rs.fetch(spec.data(), (int)spec.size()));
    }
    kb_rank::Params prm = {params[0], params[1], params[2], params[3], params[4]};
    kb_rank::Pool P = {n, slot_idx, slot_y, slot_sigma, slot_acq, slot_acq_cond, *cache_counter};
    kb_rank::Ranker rk(n, n_session, var0, prm, rs.G.data(), rs.kv.data(), &RowServer::fetch_cb, &rs, n_order + n + 1);
    const int64_t rc = rk.add(P, idx, y, sigma, acq, order, n_order);
    *cache_counter = P.cache_counter;
    if (stats) { stats[0] = rs.launches; stats[1] = rs.rows; stats[2] = rk.fetches(); }
    if (rc < 0) return ctx->err[0] ? (int)rc : gpry_fail(ctx, (int)rc, "kb_rank: the ranking failed (%lld)", (long long)rc);
    *info = rc;
    return 0;
}

}  // extern "C"
