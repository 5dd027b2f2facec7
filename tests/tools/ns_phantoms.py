"""numpy stand-ins for ``ns_generation_phantoms`` (gpry_amd/nested.py with ``phantom_thin``), and a brute-force
restatement of ``gpry_amd.nested.merged_weights``.

``PhantomNumpyDevice(loglike)``: ``ClusteredNumpyDevice`` plus ``ns_generation_phantoms``.  Every draw of a chain has a
fixed counter (generation, chain, step), so the chain of ``num_repeats = (i + 1) thin`` steps is the prefix of the longer
one: slot i of the phantoms is what the parent's ``ns_generation`` returns for that shorter walk.  Quadratic in
num_repeats, which the CPU tests' sizes bear.  ``phantom_calls`` records each call; the parent's ``calls`` keeps one
entry per generation (the full walk's).

``live_counts_brute(L, born, thr)``: the live count of every point by the definition, O(n^2): the points that have
been born and have not died when it dies."""
import numpy as np

from ns_cluster import ClusteredNumpyDevice


class PhantomNumpyDevice(ClusteredNumpyDevice):
    def __init__(self, loglike):
        super().__init__(loglike)
        self.phantom_calls = []

    def ns_generation_phantoms(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, thin,
                               labels=None, cum_p=None):
        if cum_p is not None:
            raise NotImplementedError("phantoms with cluster volumes")
        if int(thin) < 1:
            raise ValueError(f"thin = {thin}")
        kw = {} if labels is None else {"labels": labels}
        n_ph = max(num_repeats - 1, 0) // thin
        d = X_surv.shape[1]
        X_ph, y_ph = np.empty((k, n_ph, d)), np.empty((k, n_ph))
        n_calls, n_clustered = len(self.calls), self.clustered_calls
        for i in range(n_ph):
            X_ph[:, i], y_ph[:, i], _, _ = self.ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k,
                                                              (i + 1) * thin, **kw)
        del self.calls[n_calls:]
        self.clustered_calls = n_clustered
        X, y, cnt, ms = self.ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, **kw)
        self.phantom_calls.append(dict(generation=generation, k=k, lstar=lstar, thin=thin, n_ph=n_ph,
                                       clustered=labels is not None))
        return X, y, cnt, X_ph, y_ph, ms


def live_counts_brute(L, born, thr):
    """n_p of every point p (in the points' own order): the points q that are present when p dies.  Death order: the
    key (L, born, index).  q is born before p dies when it is a prior point, or its generation's threshold lies below
    L_p, or equals L_p with born_q <= born_p (ties in L are broken by generation).  q has not died when key(q) >=
    key(p); p counts itself."""
    L, born, thr = np.asarray(L, dtype=float), np.asarray(born), np.asarray(thr, dtype=float)
    n = len(L)
    key = [(L[i], born[i], i) for i in range(n)]
    out = np.zeros(n, np.int64)
    for p in range(n):
        for q in range(n):
            is_born = born[q] < 0 or thr[born[q]] < L[p] or (thr[born[q]] == L[p] and born[q] <= born[p])
            if is_born and key[q] >= key[p]:
                out[p] += 1
    return out
