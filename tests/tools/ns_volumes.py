"""numpy stand-in for the volume-weighted generation of gpry_amd/nested.py (gpry_ns_generation_volumes).

``VolumesNumpyDevice(loglike)``: ``ClusteredNumpyDevice`` plus ``ns_generation(..., labels=, cum_p=)``.  Chain c draws its
cluster q, the first q with u1 < cum_p[q] (u1: counter (START, 1, gen, c, 0)), restated with ``ns_philox.philox``; its
walk is that of the unclustered generation called with q's survivors alone (in their order) and W[q] -- the defining
property of gpry_ns_generation_volumes -- so the same u0 picks the same start.  Inputs are checked as the device checks
them."""
import numpy as np

from ns_cluster import ClusteredNumpyDevice
from ns_philox import PHASE_START, NumpyNestedDevice, philox


def drawn_clusters(seed, generation, k, cum_p):
    """The cluster each chain of a generation draws (counter (START, 1, gen, c, 0))."""
    u1, _ = philox(seed, PHASE_START, 1, generation, np.arange(k), 0)
    cum_p = np.asarray(cum_p, dtype=float)
    q = np.array([int(np.flatnonzero(u < cum_p)[0]) for u in u1], dtype=np.int64)
    return q


class VolumesNumpyDevice(ClusteredNumpyDevice):
    def __init__(self, loglike):
        super().__init__(loglike)
        self.volume_calls = []

    def ns_generation(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels=None,
                      cum_p=None):
        if cum_p is None:
            return super().ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats,
                                         labels=labels)
        W = np.asarray(W, dtype=float)
        labels = np.asarray(labels)
        cum_p = np.asarray(cum_p, dtype=float)
        nc = len(cum_p)
        if labels.min() < 0 or labels.max() >= nc:
            raise ValueError("labels outside 0 .. n_clusters - 1")
        prev = np.concatenate([[0.0], cum_p[:-1]])
        if not np.all(cum_p >= prev):
            raise ValueError("cum_p is not non-decreasing")
        if cum_p[-1] != 1.0:
            raise ValueError("the last cum_p is not 1.0")
        counts = np.bincount(labels, minlength=nc)
        if np.any((cum_p > prev) & (counts == 0)):
            raise ValueError("a cluster with positive probability has no survivor")
        q = drawn_clusters(seed, generation, k, cum_p)
        self.volume_calls.append(dict(generation=generation, n_clusters=nc, counts=counts, drawn=q))
        d = X_surv.shape[1]
        X, y, cnt = np.empty((k, d)), np.empty(k), np.zeros(k, np.int64)
        for c in np.unique(q):
            mem = np.flatnonzero(labels == c)
            Xq, yq, cq, _ = NumpyNestedDevice.ns_generation(self, lo, hi, X_surv[mem], np.asarray(y_surv)[mem], lstar,
                                                            W[c], seed, generation, k, num_repeats)
            sel = q == c
            X[sel], y[sel], cnt[sel] = Xq[sel], yq[sel], cq[sel]
        return X, y, cnt, 0.0
