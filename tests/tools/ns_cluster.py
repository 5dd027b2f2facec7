"""numpy restatement of gpry_ns_knn (gpry_amd/csrc/nested.hip) and a numpy stand-in for the clustered calls of
gpry_amd/nested.py.

``knn_table(X, lo, hi, k, rows=None)``: the device's neighbour table bit for bit -- u = (x - lo) / (hi - lo), squared
distances summed over the coordinates in their order from 0.0, each row sorted by (distance, index) with the point itself
left out.  ``rows``: only those rows (the whole table of a large set does not fit in memory at once).

``ClusteredNumpyDevice(loglike)``: ``NumpyNestedDevice`` plus ``ns_knn`` and ``ns_generation(..., labels=)``.  Its
clustered generation is built from the unclustered one by the defining property of gpry_ns_generation_clustered: one
call per cluster's W, of which the chains that start in that cluster are kept."""
import numpy as np

from ns_philox import PHASE_START, NumpyNestedDevice, philox


def knn_table(X, lo, hi, k, rows=None, block=256):
    X = np.asarray(X, dtype=float)
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    U = (X - lo) / (hi - lo)
    n, d = U.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), k), dtype=np.int32)
    for b in range(0, len(rows), block):
        r = rows[b:b + block]
        D = np.zeros((len(r), n))
        for c in range(d):
            df = U[r, c][:, None] - U[None, :, c]
            D = D + df * df
        order = np.argsort(D, axis=-1, kind="stable")          # (equal distances: by index)
        keep = order != r[:, None]
        out[b:b + block] = order[keep].reshape(len(r), n - 1)[:, :k]
    return out


def chain_starts(seed, generation, k, nsurv):
    """The survivor each chain of a generation starts from (counter (START, 0, gen, c, 0))."""
    us, _ = philox(seed, PHASE_START, 0, generation, np.arange(k), 0)
    return np.minimum((us * nsurv).astype(np.int64), nsurv - 1)


class ClusteredNumpyDevice(NumpyNestedDevice):
    def __init__(self, loglike):
        super().__init__(loglike)
        self.knn_calls = []
        self.clustered_calls = 0

    def ns_knn(self, lo, hi, X, k):
        self.knn_calls.append(dict(n=len(X), k=k))
        return knn_table(X, lo, hi, k), 0.0

    def ns_generation(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels=None):
        if labels is None:
            return super().ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats)
        W = np.asarray(W, dtype=float)
        start = np.asarray(labels)[chain_starts(seed, generation, k, len(X_surv))]
        d = X_surv.shape[1]
        X, y, cnt = np.empty((k, d)), np.empty(k), np.zeros(k, np.int64)
        for q in np.unique(start):
            Xq, yq, cq, _ = super().ns_generation(lo, hi, X_surv, y_surv, lstar, W[q], seed, generation, k, num_repeats)
            sel = start == q
            X[sel], y[sel], cnt[sel] = Xq[sel], yq[sel], cq[sel]
        self.clustered_calls += 1
        return X, y, cnt, 0.0
