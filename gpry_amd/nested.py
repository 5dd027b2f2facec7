"""Nested sampling of the surrogate's posterior mean, with the likelihood evaluated on the device.

The reference draws NORA's candidate pool with PolyChord or UltraNest (gpry/gp_acquisition.py:650-682, 760-856), which
call ``gpr.predict`` once per point.  Here the evaluations run in two HIP kernels (``gpry_amd/csrc/nested.hip``): one
that draws and evaluates the prior points, one that runs a whole generation of slice-sampling chains.  This module
keeps the bookkeeping: the live set, prior volumes, the whitening matrix of the chains, the stopping rule, the weights
and the evidence.  It talks to the device only through two calls, so any object with the same two methods can stand in
for it (the CPU tests use a numpy one):

``dev.ns_prior(lo, hi, seed, n) -> (X (n, d), y (n,), device_ms)``
``dev.ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats)
    -> (X_new (k, d), y_new (k,), ncalls (k,), device_ms)``

With ``clustering=True`` it also calls ``dev.ns_knn(lo, hi, X, k) -> (nbr (n, k), device_ms)`` and passes
``labels=`` (with one W per cluster) to ``ns_generation``.

The algorithm, step by step:

* The sampler works in the unit cube u = (x - lo) / (hi - lo); the prior is uniform on the box.
* A point is outside when its y is -inf, or <= ``minus_inf_value`` if that is finite; its likelihood is then zero.
* Start: ``nprior`` uniform points, all live.  The lowest are removed one at a time until ``nlive`` remain.
* Generation: the live set sorted by (y, index), the ``batch`` lowest become dead points in ascending order, L* is the
  largest y among them, and as many chains, each started from a uniformly drawn survivor, produce one new live point
  above L*.  Every removal with n live points before it shrinks the log prior volume by log(n / (n + 1)).
* Clustering (opt-in): after the kill, the survivors' k-nearest-neighbour table (device) is cut into clusters by
  ``knn_clusters``, each cluster gets the whitening matrix of its own points, and every chain walks with the matrix of
  the cluster its start belongs to.  Starts, kills and volumes are those of the unclustered run, so a cluster receives
  new points in proportion to its live count and logZ and the weights keep their meaning.  Not done: PolyChord's
  per-cluster volumes and local evidences, and the choice of a cluster in proportion to its volume.
* Stop when Z_live / Z < ``precision_criterion`` (Z_live = X mean(L_live), the PolyChord criterion) or, at the end of
  a generation, when the evaluation count has reached ``max_ncalls``.  The final live points get the volume X / n each.
"""
from collections import namedtuple
from time import time

import numpy as np

NestedResult = namedtuple("NestedResult", ["X", "y", "w", "logZ", "logZ_err", "ncalls", "ngen", "device_s",
                                           "wall_s", "dead_L", "dead_logX", "n_dead", "n_clusters"],
                          defaults=(None,))
NestedResult.__doc__ = """Output of ``run_nested``.  X, y, w: rows with a finite likelihood, dead points in the order they
died then the final live points; w sums to 1.  logZ and its error sqrt(H / nlive); ncalls: evaluations of the surrogate;
ngen: generations; device_s / wall_s: time in the device calls / in the whole run.  dead_L / dead_logX: log-likelihood
(-inf outside) and log prior volume after each removal, outside points included; n_dead: their count.  n_clusters: the
cluster count of each generation (an int array) with clustering on, None without."""

# a run stops after this many generations whatever its other criteria say (a safeguard, never met in practice)
MAX_GENERATIONS = 100000
# largest neighbour count the clustering rule tries (profiles/nested_clusters.md)
DEFAULT_CLUSTER_K_MAX = 10


def default_batch(nlive):
    """Chains per generation when the caller does not choose: nlive / 2 (profiles/r07_nested.md)."""
    return max(1, int(nlive) // 2)


def whitening(U):
    """Lower Cholesky factor of the covariance of the rows of U (unit-cube coordinates), with a growing ridge while the
    covariance is singular."""
    U = np.asarray(U, dtype=float)
    d = U.shape[1]
    C = np.atleast_2d(np.cov(U, rowvar=False, ddof=0)) if len(U) > 1 else np.zeros((d, d))
    return cholesky_ridged(C)


def cholesky_ridged(C):
    """Lower Cholesky factor of the covariance matrix C, with a growing ridge while C is singular."""
    C = np.atleast_2d(np.asarray(C, dtype=float))
    d = C.shape[0]
    scale = max(float(np.trace(C)) / d, 1e-12)
    ridge = 0.0
    for _ in range(30):
        try:
            return np.ascontiguousarray(np.linalg.cholesky(C + ridge * np.eye(d)))
        except np.linalg.LinAlgError:
            ridge = scale * 1e-12 if ridge == 0.0 else ridge * 100.0
    return np.ascontiguousarray(np.sqrt(scale) * np.eye(d))


def _components(n, a, b):
    """Connected components of the graph on 0 .. n-1 with the edges a[e]-b[e]: each point's smallest component member.
    Union-find with the roots as the smaller index, vectorised: every edge hooks the larger of its two roots onto the
    smaller, then the paths are compressed, until both ends of every edge share a root."""
    parent = np.arange(n)
    while True:
        ra, rb = parent[a], parent[b]
        if np.array_equal(ra, rb):
            return parent
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def knn_clusters(nbr, d, k_max, min_size=None):
    """Clusters of a live set from its neighbour table ``nbr`` (n, >= k_max; row i: i's nearest other points, nearest
    first): ``(labels (n,) int32, n_clusters)``.

    For k = 2 .. k_max: the undirected graph with an edge i-j when j is among the first k neighbours of i or i among
    those of j, and its connected components, numbered by their smallest member.  The partition is the first one at a
    k >= 3 that equals the one at k - 1; a single component ends the search at once.  If no partition is stable up to
    k_max, or a cluster has fewer than ``min_size`` points (default d + 1: too few for a covariance), it is one cluster.
    After PolyChord's KNN clustering (Handley et al. 2015), without claiming to be it bit for bit."""
    nbr = np.asarray(nbr)
    n = nbr.shape[0]
    one = (np.zeros(n, np.int32), 1)
    k_max = min(int(k_max), nbr.shape[1] if nbr.ndim == 2 else 0)
    min_size = int(d) + 1 if min_size is None else int(min_size)
    prev = None
    for k in range(2, k_max + 1):
        a = np.repeat(np.arange(n), k)
        roots = _components(n, a, nbr[:, :k].reshape(-1).astype(np.int64))
        _, labels = np.unique(roots, return_inverse=True)
        if labels.max() == 0:
            return one
        if prev is not None and np.array_equal(labels, prev):
            counts = np.bincount(labels)
            if counts.min() < min_size:
                return one
            return labels.astype(np.int32), len(counts)
        prev = labels
    return one


def _logL(y, minus_inf_value):
    L = np.asarray(y, dtype=float).copy()
    if np.isfinite(minus_inf_value):
        L[L <= minus_inf_value] = -np.inf
    return L


def _logsumexp(a):
    a = np.asarray(a, dtype=float)
    if a.size == 0:
        return -np.inf
    m = np.max(a)
    if not np.isfinite(m):
        return m
    return m + np.log(np.sum(np.exp(a - m)))


def run_nested(dev, bounds, seed, nlive, num_repeats, precision_criterion=0.01, nprior=None, max_ncalls=None,
               batch=None, minus_inf_value=-np.inf, clustering=False, cluster_k_max=None):
    """Nested sampling run of the surrogate on ``dev``; see the module's docstring.  Returns a ``NestedResult``.
    ``clustering``: a whitening matrix per cluster of the survivors (``knn_clusters`` with neighbour tables of up to
    ``cluster_k_max`` points, default ``DEFAULT_CLUSTER_K_MAX``)."""
    t_start = time()
    bounds = np.asarray(bounds, dtype=float)
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    nlive = int(nlive)
    if nlive < 2:
        raise ValueError(f"nlive = {nlive}: at least 2 live points are needed")
    nprior = nlive if nprior is None else max(int(nprior), nlive)
    k_gen = default_batch(nlive) if batch is None else int(batch)
    if not 1 <= k_gen <= nlive - 1:
        raise ValueError(f"batch = {k_gen} must lie in 1 .. nlive - 1 = {nlive - 1}")
    num_repeats = int(num_repeats)
    seed = int(seed)
    clustering = bool(clustering)
    k_max = DEFAULT_CLUSTER_K_MAX if cluster_k_max is None else int(cluster_k_max)
    if clustering and not 2 <= k_max <= 32:
        raise ValueError(f"cluster_k_max = {k_max} must lie in 2 .. 32")
    n_clusters = []
    device_ms = 0.0
    # ---- prior
    X, y, ms = dev.ns_prior(lo, hi, seed, nprior)
    device_ms += ms
    ncalls = nprior
    L = _logL(y, minus_inf_value)
    dead_X, dead_y, dead_L, dead_logw, dead_logX = [], [], [], [], []
    logX = 0.0

    def kill(idx, Xl, yl, Ll, logX):
        """idx: positions of the removed points in ascending order; returns the new log volume."""
        n = len(Ll)
        nb = n - np.arange(len(idx), dtype=float)                 # live count before each removal
        logX_seq = logX + np.cumsum(np.log(nb / (nb + 1.0)))
        logX_prev = np.concatenate([[logX], logX_seq[:-1]])
        # w_i = L_i (X_{i-1} - X_i) = L_i X_{i-1} / (n + 1)
        with np.errstate(invalid="ignore"):
            logw = Ll[idx] + logX_prev - np.log(nb + 1.0)
        logw[~np.isfinite(Ll[idx])] = -np.inf
        dead_X.append(Xl[idx]); dead_y.append(yl[idx]); dead_L.append(Ll[idx])
        dead_logw.append(logw); dead_logX.append(logX_seq)
        return float(logX_seq[-1]) if len(idx) else logX

    def order_of(Ll):
        return np.lexsort((np.arange(len(Ll)), Ll))

    if nprior > nlive:
        order = order_of(L)
        logX = kill(order[:nprior - nlive], X, y, L, logX)
        keep = np.sort(order[nprior - nlive:])
        X, y, L = X[keep], y[keep], L[keep]
    gen = 0
    while True:
        logZ_dead = _logsumexp(np.concatenate(dead_logw)) if dead_logw else -np.inf
        logZ_live = logX + _logsumexp(L) - np.log(len(L))
        logZ = np.logaddexp(logZ_dead, logZ_live)
        if not np.isfinite(logZ) or logZ_live - logZ < np.log(precision_criterion):
            break
        if max_ncalls is not None and ncalls >= max_ncalls:
            break
        if gen >= MAX_GENERATIONS:
            break
        order = order_of(L)
        rem, keep = order[:k_gen], np.sort(order[k_gen:])
        lstar = float(L[rem[-1]])
        logX = kill(rem, X, y, L, logX)
        Xs, ys = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
        Us = (Xs - lo) / (hi - lo)
        # an outside point is never accepted: with a finite minus_inf_value the threshold is at least that value
        thr = lstar if not np.isfinite(minus_inf_value) else max(lstar, float(minus_inf_value))
        if not clustering:
            W = whitening(Us)
            Xn, yn, cnt, ms = dev.ns_generation(lo, hi, Xs, ys, thr, W, seed, gen, k_gen, num_repeats)
        else:
            if len(Xs) >= 3:
                nbr, ms = dev.ns_knn(lo, hi, Xs, min(k_max, len(Xs) - 1))
                device_ms += ms
                labels, nc = knn_clusters(nbr, Xs.shape[1], k_max)
            else:
                labels, nc = np.zeros(len(Xs), np.int32), 1
            W = np.stack([whitening(Us[labels == q]) for q in range(nc)])
            n_clusters.append(nc)
            Xn, yn, cnt, ms = dev.ns_generation(lo, hi, Xs, ys, thr, W, seed, gen, k_gen, num_repeats, labels=labels)
        device_ms += ms
        ncalls += int(np.sum(cnt))
        X = np.concatenate([Xs, Xn])
        y = np.concatenate([ys, yn])
        L = np.concatenate([L[keep], _logL(yn, minus_inf_value)])
        gen += 1
    # ---- final live points: volume X / n each
    n = len(L)
    live_logw = L + logX - np.log(n)
    all_X = np.concatenate(dead_X + [X]) if dead_X else X
    all_y = np.concatenate(dead_y + [y]) if dead_y else y
    all_L = np.concatenate(dead_L + [L]) if dead_L else L
    all_logw = np.concatenate(dead_logw + [live_logw]) if dead_logw else live_logw
    logZ = _logsumexp(all_logw)
    fin = np.isfinite(all_L)
    if np.isfinite(logZ):
        p = np.exp(all_logw[fin] - logZ)
        H = float(np.sum(p * (all_L[fin] - logZ)))
        w = p / np.sum(p)
    else:
        H, w = 0.0, np.zeros(int(fin.sum()))
    return NestedResult(X=np.ascontiguousarray(all_X[fin]), y=np.ascontiguousarray(all_y[fin]), w=w, logZ=float(logZ),
                        logZ_err=float(np.sqrt(max(H, 0.0) / nlive)), ncalls=int(ncalls), ngen=gen,
                        device_s=device_ms / 1e3, wall_s=time() - t_start,
                        dead_L=np.concatenate(dead_L) if dead_L else np.empty(0),
                        dead_logX=np.concatenate(dead_logX) if dead_logX else np.empty(0),
                        n_dead=int(sum(len(a) for a in dead_y)),
                        n_clusters=np.array(n_clusters, dtype=np.int64) if clustering else None)
