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
``labels=`` (with one W per cluster) to ``ns_generation``; with ``cluster_volumes=True`` as well, it passes ``cum_p=``
(cumulative cluster probabilities) too.  With ``phantom_thin`` it calls, in place of ``ns_generation``,

``dev.ns_generation_phantoms(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, thin, labels=None)
    -> (X_new, y_new, ncalls, X_ph (k, n_ph, d), y_ph (k, n_ph), device_ms)``

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
  new points in proportion to its live count and logZ and the weights keep their meaning.
* Per-cluster volumes (opt-in on top of clustering, after PolyChord, Handley et al. 2015): every cluster q keeps its own
  log volume log X_q and live count n_q.  The kills are those above (the lowest of the whole live set), but a point
  that dies in q weighs L X_q / (n_q + 1) and shrinks X_q by n_q / (n_q + 1); an emptied cluster is closed and the rest
  of its volume dropped.  After the kill each open cluster's survivors are clustered on their own (clusters only
  split); a split closes q and gives each child X_q n_child / n_q.  Every chain draws its cluster in proportion to X_q
  (``chain_clusters`` restates the device's draw), its start uniformly among that cluster's survivors, and its new
  point joins that cluster.  Z_live = sum_q X_q mean(L over q); the final live points of q get X_q / n_q each.  Every row records its
  cluster id; the local evidence of an id sums the weights of its rows, and a mode's evidence is the sum over its
  subtree (profiles/nested_volumes.md).
* Phantoms (opt-in, ``phantom_thin``; after PolyChord's ``boost_posterior``): every thin-th interior state of a chain is
  kept as well.  A chain starts from a live point, which is uniform in {L > L*}, and a slice-sampling step leaves that
  distribution invariant, so every state is a (correlated) sample of the contour it was born in.  The run itself does
  not see them: kills, thresholds, stopping, logZ, its error and the real rows are those of the run without.  They are
  appended to the rows and all rows are weighted by ``merged_weights``, which treats the points like the threads of a
  dynamic nested-sampling run (Higson et al. 2019): the live count becomes a function of the likelihood level.  Not
  available together with ``cluster_volumes``: per-cluster birth volumes are not kept.
* Stop when Z_live / Z < ``precision_criterion`` (Z_live = X mean(L_live), the PolyChord criterion) or, at the end of
  a generation, when the evaluation count has reached ``max_ncalls``.  The final live points get the volume X / n each.
"""
from collections import defaultdict, namedtuple
from time import time

import numpy as np

NestedResult = namedtuple("NestedResult", ["X", "y", "w", "logZ", "logZ_err", "ncalls", "ngen", "device_s",
                                           "wall_s", "dead_L", "dead_logX", "n_dead", "n_clusters", "cluster",
                                           "cluster_logZ", "cluster_parent", "phantom", "logZ_merged", "n_phantom"],
                          defaults=(None, None, None, None, None, None, None))
NestedResult.__doc__ = """Output of ``run_nested``.  X, y, w: rows with a finite likelihood, dead points in the order they
died then the final live points; w sums to 1.  logZ and its error sqrt(H / nlive); ncalls: evaluations of the surrogate;
ngen: generations; device_s / wall_s: time in the device calls / in the whole run.  dead_L / dead_logX: log-likelihood
(-inf outside) and log prior volume after each removal, outside points included; n_dead: their count.  n_clusters: the
cluster count of each generation (an int array) with clustering on, None without.  With cluster_volumes on (None
without): cluster, the id of the cluster each row of X died or stayed live in; cluster_logZ, the local evidence of each
id (log of the summed weights of its rows, unnormalised: their logsumexp is logZ); cluster_parent, each id's parent id
(-1 for the root).  dead_logX is then the log of the summed volume of the open clusters.  With phantom_thin (None
without): phantom, True for the rows that are phantoms (they follow the real rows, in (generation, chain, slot) order);
logZ_merged, the evidence of the merged point set (``merged_weights``); n_phantom, the count of phantom rows.  w then
comes from ``merged_weights`` and covers all rows; logZ and logZ_err remain those of the run."""

# a run stops after this many generations whatever its other criteria say (a safeguard, never met in practice)
MAX_GENERATIONS = 100000
# largest neighbour count the clustering rule tries (profiles/nested_clusters.md)
DEFAULT_CLUSTER_K_MAX = 10
# Philox4x32-10 of nested.hip: the multipliers and key increments, and the phase of a chain's start draws
_PH_M0, _PH_M1, _PH_W0, _PH_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_PHASE_START = 1


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


def _philox_a(seed, word0, gen, chain, step):
    """Word a of the device's ns_philox for the counters (word0, gen, chain, step), vectorised over ``chain``: a uniform
    in [0, 1) with 53 bits."""
    m = np.uint64(0xFFFFFFFF)
    c1 = np.full(np.shape(chain), gen, np.uint64) & m
    c0 = np.full_like(c1, word0) & m
    c2 = np.asarray(chain, dtype=np.uint64) & m
    c3 = np.full_like(c1, step) & m
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PH_M0) * c0, np.uint64(_PH_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(_PH_W0)) & m, (k1 + np.uint64(_PH_W1)) & m
    return (((c0 << np.uint64(32)) | c1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def chain_clusters(seed, generation, k, cum_p):
    """The cluster each of the ``k`` chains of a generation draws in ``ns_generation(..., cum_p=)``
    (gpry_ns_generation_volumes): the first q with u1 < cum_p[q], u1 from the counter (START, 1, generation, c, 0)."""
    u1 = _philox_a(int(seed), (_PHASE_START << 24) | 1, int(generation), np.arange(int(k)), 0)
    cum_p = np.asarray(cum_p, dtype=float)
    return np.minimum(np.searchsorted(cum_p, u1, side="right"), len(cum_p) - 1)


def cluster_probabilities(logX):
    """Cumulative probabilities of choosing each cluster in proportion to its volume exp(logX), non-decreasing, the last
    exactly 1.0."""
    logX = np.asarray(logX, dtype=float)
    cum = np.minimum(np.cumsum(np.exp(logX - _logsumexp(logX))), 1.0)
    cum[-1] = 1.0
    return cum


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


def merged_weights(L, born, thr, L_end=None):
    """Log weights of a point set in which every point is uniform in the contour it was born in: ``(logw (n,), logZ)``.

    ``L`` (n,): log-likelihoods, -inf outside.  ``born`` (n,): the generation a point was born in, -1 for a prior point.
    ``thr`` (G,): the threshold of each generation, non-decreasing; a point of generation g lies in {L > thr[g]} (or at
    thr[g], where a plateau lets a chain stay on its start).  ``L_end``: points above it form the final set (default:
    thr[-1], or -inf without generations).

    All points, outside ones included, are ordered by (L, born, row index).  The point at position r (from 0) has the
    live count n_r = B_r - r, where B_r = #prior + sum of m_g over the generations counted as born by then: those with
    thr[g] < L_r and, among those with thr[g] == L_r, the ones with g <= born_r (m_g: the points born in g).  Ties in L
    are thus broken by generation, and a generation whose threshold equals L_r is counted once the order has reached its
    own points; every point sorted up to r then belongs to a counted generation, so n_r >= 1 also on a plateau of tied
    values (a count is still clamped to 1, which only an outside start that never moved can need).  Points with
    L <= L_end die in that order: log X_r = sum_{j <= r} log(n_j / (n_j + 1)), log w_r = L_r + log X_{r-1} -
    log(n_r + 1).  The n_final points above L_end get X_end / n_final each.  Outside points weigh 0.  With one
    generation's worth of new live points per threshold and no ties this is the run's own weighting."""
    L = np.asarray(L, dtype=float)
    born = np.asarray(born, dtype=np.int64)
    thr = np.asarray(thr, dtype=float)
    n, G = len(L), len(thr)
    if born.shape != L.shape or (n and (born.min() < -1 or born.max() >= G)):
        raise ValueError("born must hold one generation in -1 .. len(thr) - 1 per point")
    if np.any(thr[1:] < thr[:-1]):
        raise ValueError("thr must be non-decreasing")
    if L_end is None:
        L_end = thr[-1] if G else -np.inf
    order = np.lexsort((np.arange(n), born, L))
    Ls, bs = L[order], born[order]
    cum_m = np.concatenate([[0], np.cumsum(np.bincount(born[born >= 0], minlength=G))])
    below, upto = np.searchsorted(thr, Ls, side="left"), np.searchsorted(thr, Ls, side="right")
    B = int(np.count_nonzero(born < 0)) + cum_m[np.maximum(below, np.minimum(upto, bs + 1))]
    cnt = np.maximum(B - np.arange(n), 1).astype(float)
    nd = int(np.searchsorted(Ls, L_end, side="right"))          # the first nd die in order
    logX = np.cumsum(np.log(cnt[:nd] / (cnt[:nd] + 1.0)))
    logX_prev = np.concatenate([[0.0], logX[:-1]])
    logw_s = np.empty(n)
    with np.errstate(invalid="ignore"):
        logw_s[:nd] = Ls[:nd] + logX_prev - np.log(cnt[:nd] + 1.0)
        if n > nd:
            logw_s[nd:] = Ls[nd:] + (logX[-1] if nd else 0.0) - np.log(n - nd)
    logw_s[~np.isfinite(Ls)] = -np.inf
    logw = np.empty(n)
    logw[order] = logw_s
    return logw, float(_logsumexp(logw))


def _prior_phase(dev, lo, hi, seed, nprior, minus_inf_value):
    """The start of a run: ``nprior`` uniform points, ``(X, y, L, device_ms)``."""
    X, y, ms = dev.ns_prior(lo, hi, seed, nprior)
    return X, y, _logL(y, minus_inf_value), ms


def _split(L, k, minus_inf_value):
    """The kill of the ``k`` lowest of a live set ordered by (L, index): ``(rem, keep, thr)``, the positions of the
    removed points in that order, those of the survivors in ascending order, and the threshold L* for the new points."""
    order = np.lexsort((np.arange(len(L)), L))
    rem, keep = order[:k], np.sort(order[k:])
    lstar = float(L[rem[-1]])
    # an outside point is never accepted: with a finite minus_inf_value the threshold is at least that value
    return rem, keep, lstar if not np.isfinite(minus_inf_value) else max(lstar, float(minus_inf_value))


def _goes_on(dead, logZ_live, precision_criterion, ncalls, max_ncalls, gen):
    """The stopping rule, asked before every generation: False once Z_live / Z < precision_criterion (or Z is not finite),
    the evaluations have reached ``max_ncalls``, or after MAX_GENERATIONS."""
    logZ = np.logaddexp(_logsumexp(np.concatenate(dead["logw"])) if dead["logw"] else -np.inf, logZ_live)
    if not np.isfinite(logZ) or logZ_live - logZ < np.log(precision_criterion):
        return False
    return not (max_ncalls is not None and ncalls >= max_ncalls) and gen < MAX_GENERATIONS


def _bury(dead, **columns):
    """Appends one kill's arrays (X, y, L, logw, logX, ...) to the lists of the dead points."""
    for name, a in columns.items():
        dead[name].append(a)


def _clusters_of(dev, lo, hi, Xs, k_max):
    """``(labels, n_clusters, device_ms)`` of the points Xs: the device's neighbour table cut by ``knn_clusters``; fewer
    than 3 points are one cluster."""
    if len(Xs) < 3:
        return np.zeros(len(Xs), np.int32), 1, 0.0
    nbr, ms = dev.ns_knn(lo, hi, Xs, min(k_max, len(Xs) - 1))
    return knn_clusters(nbr, Xs.shape[1], k_max) + (ms,)


def _generation(dev, thin, *args, **kw):
    """The run loops' one way to the device: ``dev.ns_generation(*args, **kw)``, or with ``thin`` (phantoms)
    ``dev.ns_generation_phantoms(*args, thin, **kw)``: ``(X_new, y_new, ncalls, X_ph, y_ph, device_ms)``, X_ph and y_ph
    None without ``thin``."""
    if thin is not None:
        return dev.ns_generation_phantoms(*args, thin, **kw)
    Xn, yn, cnt, ms = dev.ns_generation(*args, **kw)
    return Xn, yn, cnt, None, None, ms


def _finish(dead, X, y, L, live_logw, nlive, ncalls, gen, device_ms, n_clusters):
    """The end of a run: the dead points in the order they died, then the final live ones with the log weights
    ``live_logw``; logZ, the information H and w from all of them.  Returns the fields of ``NestedResult`` that every
    run has (rows: the points with a finite likelihood) and, for all points, L and the log weights."""
    all_X, all_y, all_L, all_logw = (np.concatenate(dead[name] + [live])
                                     for name, live in (("X", X), ("y", y), ("L", L), ("logw", live_logw)))
    logZ = _logsumexp(all_logw)
    fin = np.isfinite(all_L)
    if np.isfinite(logZ):
        p = np.exp(all_logw[fin] - logZ)
        H = float(np.sum(p * (all_L[fin] - logZ)))
        w = p / np.sum(p)
    else:
        H, w = 0.0, np.zeros(int(fin.sum()))
    res = dict(X=np.ascontiguousarray(all_X[fin]), y=np.ascontiguousarray(all_y[fin]), w=w, logZ=float(logZ),
               logZ_err=float(np.sqrt(max(H, 0.0) / nlive)), ncalls=int(ncalls), ngen=gen, device_s=device_ms / 1e3,
               dead_L=np.concatenate(dead["L"]) if dead["L"] else np.empty(0),
               dead_logX=np.concatenate(dead["logX"]) if dead["logX"] else np.empty(0),
               n_dead=int(sum(len(a) for a in dead["y"])),
               n_clusters=None if n_clusters is None else np.array(n_clusters, dtype=np.int64))
    return res, all_L, all_logw


def _with_phantoms(res, all_L, n_live, born, thrs, ph_X, ph_y, d, minus_inf_value):
    """The fields of a run with phantoms from those without (``res``): the real rows, then the phantoms in (generation,
    chain, slot) order, all of them weighted as one merged run.  ``all_L``, ``born``: of all real points, the last
    ``n_live`` of them live; ``thrs``: each generation's threshold; ``ph_X`` / ``ph_y``: each generation's phantoms."""
    Xp = np.concatenate(ph_X) if ph_X else np.empty((0, d))
    yp = np.concatenate(ph_y) if ph_y else np.empty(0)
    per_gen = len(ph_y[0]) if ph_y else 0
    m_L = np.concatenate([all_L, _logL(yp, minus_inf_value)])
    m_born = np.concatenate([born, np.repeat(np.arange(len(thrs), dtype=np.int64), per_gen)])
    n_dead_all = len(all_L) - n_live
    L_end = float(all_L[n_dead_all - 1]) if n_dead_all else -np.inf
    logw_m, logZ_m = merged_weights(m_L, m_born, np.array(thrs, dtype=float), L_end=L_end)
    fin_m = np.isfinite(m_L)
    if np.isfinite(logZ_m):
        w = np.exp(logw_m[fin_m] - logZ_m)
        w = w / np.sum(w)
    else:
        w = np.zeros(int(fin_m.sum()))
    fin_p = fin_m[len(all_L):]
    flag = np.zeros(len(res["y"]) + int(fin_p.sum()), bool)
    flag[len(res["y"]):] = True
    return dict(res, X=np.ascontiguousarray(np.concatenate([res["X"], Xp[fin_p]])),
                y=np.ascontiguousarray(np.concatenate([res["y"], yp[fin_p]])), w=w, phantom=flag, logZ_merged=logZ_m,
                n_phantom=int(fin_p.sum()))


def run_nested(dev, bounds, seed, nlive, num_repeats, precision_criterion=0.01, nprior=None, max_ncalls=None,
               batch=None, minus_inf_value=-np.inf, clustering=False, cluster_k_max=None, cluster_volumes=False,
               phantom_thin=None):
    """Nested sampling run of the surrogate on ``dev``; see the module's docstring.  Returns a ``NestedResult``.
    ``clustering``: a whitening matrix per cluster of the survivors (``knn_clusters`` with neighbour tables of up to
    ``cluster_k_max`` points, default ``DEFAULT_CLUSTER_K_MAX``).  ``cluster_volumes`` (needs ``clustering``): every
    cluster keeps its own prior volume and local evidence, and chains start in a cluster drawn by volume.
    ``phantom_thin`` (None: off; an int >= 1): keep every thin-th interior state of the chains as a weighted phantom row
    (``dev.ns_generation_phantoms``); the run is the one without, the rows grow and ``w`` comes from ``merged_weights``.
    Not together with ``cluster_volumes`` (ValueError): the phantoms' per-cluster birth volumes are not kept."""
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
    if phantom_thin is not None:
        if isinstance(phantom_thin, bool) or int(phantom_thin) != phantom_thin or int(phantom_thin) < 1:
            raise ValueError(f"phantom_thin = {phantom_thin!r} must be an int >= 1 (or None)")
        phantom_thin = int(phantom_thin)
        if cluster_volumes:
            raise ValueError("phantom_thin with cluster_volumes=True: phantoms have no per-cluster birth volumes")
    if cluster_volumes:
        if not clustering:
            raise ValueError("cluster_volumes=True needs clustering=True")
        res = _run_volumes(dev, lo, hi, seed, nlive, nprior, k_gen, num_repeats, precision_criterion, max_ncalls,
                           minus_inf_value, k_max)
    else:
        res = _run_one_volume(dev, lo, hi, seed, nlive, nprior, k_gen, num_repeats, precision_criterion, max_ncalls,
                              minus_inf_value, k_max if clustering else None, phantom_thin)
    return NestedResult(wall_s=time() - t_start, **res)


def _run_one_volume(dev, lo, hi, seed, nlive, nprior, k_gen, num_repeats, precision_criterion, max_ncalls,
                    minus_inf_value, k_max, phantom_thin):
    """The run with one prior volume for the whole live set: plain, with a whitening matrix per cluster (``k_max`` not
    None) and / or with phantoms (``phantom_thin`` not None).  Returns the fields of the ``NestedResult``."""
    X, y, L, device_ms = _prior_phase(dev, lo, hi, seed, nprior, minus_inf_value)
    ncalls, logX, n_clusters, dead = nprior, 0.0, [], defaultdict(list)
    # for the phantoms' weights: the generation every point was born in (-1: prior), each generation's threshold, phantoms
    born, thrs, ph_X, ph_y = np.full(nprior, -1, np.int64), [], [], []

    def kill(idx):
        """idx: positions of the removed points in ascending order; returns the new log volume."""
        nb = len(L) - np.arange(len(idx), dtype=float)             # live count before each removal
        logX_seq = logX + np.cumsum(np.log(nb / (nb + 1.0)))
        logX_prev = np.concatenate([[logX], logX_seq[:-1]])
        # w_i = L_i (X_{i-1} - X_i) = L_i X_{i-1} / (n + 1)
        with np.errstate(invalid="ignore"):
            logw = L[idx] + logX_prev - np.log(nb + 1.0)
        logw[~np.isfinite(L[idx])] = -np.inf
        _bury(dead, X=X[idx], y=y[idx], L=L[idx], logw=logw, logX=logX_seq, born=born[idx])
        return float(logX_seq[-1]) if len(idx) else logX

    if nprior > nlive:
        rem, keep, _ = _split(L, nprior - nlive, minus_inf_value)
        logX = kill(rem)
        X, y, L, born = X[keep], y[keep], L[keep], born[keep]
    gen = 0
    while _goes_on(dead, logX + _logsumexp(L) - np.log(len(L)), precision_criterion, ncalls, max_ncalls, gen):
        rem, keep, thr = _split(L, k_gen, minus_inf_value)
        logX = kill(rem)
        Xs, ys = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
        Us = (Xs - lo) / (hi - lo)
        thrs.append(thr)
        if k_max is None:
            W, kw = whitening(Us), {}
        else:
            labels, nc, ms = _clusters_of(dev, lo, hi, Xs, k_max)
            device_ms += ms
            W, kw = np.stack([whitening(Us[labels == q]) for q in range(nc)]), {"labels": labels}
            n_clusters.append(nc)
        Xn, yn, cnt, Xp, yp, ms = _generation(dev, phantom_thin, lo, hi, Xs, ys, thr, W, seed, gen, k_gen, num_repeats,
                                              **kw)
        if phantom_thin is not None:
            ph_X.append(np.asarray(Xp, dtype=float).reshape(-1, len(lo)))
            ph_y.append(np.asarray(yp, dtype=float).reshape(-1))
        device_ms += ms
        ncalls += int(np.sum(cnt))
        X = np.concatenate([Xs, Xn])
        y = np.concatenate([ys, yn])
        L = np.concatenate([L[keep], _logL(yn, minus_inf_value)])
        born = np.concatenate([born[keep], np.full(k_gen, gen, np.int64)])
        gen += 1
    # the final live points: volume X / n each
    res, all_L, _ = _finish(dead, X, y, L, L + logX - np.log(len(L)), nlive, ncalls, gen, device_ms,
                            None if k_max is None else n_clusters)
    if phantom_thin is None:
        return res
    return _with_phantoms(res, all_L, len(L), np.concatenate(dead["born"] + [born]), thrs, ph_X, ph_y, len(lo),
                          minus_inf_value)


def _run_volumes(dev, lo, hi, seed, nlive, nprior, k_gen, num_repeats, precision_criterion, max_ncalls, minus_inf_value,
                 k_max):
    """run_nested(clustering=True, cluster_volumes=True): the module docstring's per-cluster bookkeeping.  Returns the
    fields of the ``NestedResult``."""
    d = len(lo)
    X, y, L, device_ms = _prior_phase(dev, lo, hi, seed, nprior, minus_inf_value)
    ncalls, n_clusters, dead = nprior, [], defaultdict(list)
    cl = np.zeros(len(L), np.int64)                 # the cluster id of every live point
    parent, logXc = [-1], [0.0]                     # per id: parent id, log prior volume
    open_ids = [0]

    def kill(idx):
        """idx: positions of the removed points in ascending (y, index) order.  Every cluster's volume shrinks by
        n_q / (n_q + 1) per removal of one of its n_q live points."""
        cid = cl[idx]
        logw = np.empty(len(idx))
        touched = np.unique(cid)
        after = np.empty((len(idx), len(touched)))  # log volume of each touched cluster after each removal
        for col, q in enumerate(touched):
            sel = np.flatnonzero(cid == q)
            nb = np.count_nonzero(cl == q) - np.arange(len(sel), dtype=float)
            seq = logXc[q] + np.cumsum(np.log(nb / (nb + 1.0)))
            prev = np.concatenate([[logXc[q]], seq[:-1]])
            with np.errstate(invalid="ignore"):
                logw[sel] = L[idx[sel]] + prev - np.log(nb + 1.0)
            seen = np.cumsum(cid == q)
            after[:, col] = np.where(seen > 0, seq[np.maximum(seen - 1, 0)], logXc[q])
            logXc[q] = float(seq[-1])
        logw[~np.isfinite(L[idx])] = -np.inf
        rest = [logXc[q] for q in open_ids if q not in touched]
        if rest:
            after = np.concatenate([after, np.broadcast_to(np.array(rest), (len(idx), len(rest)))], axis=1)
        mx = np.max(after, axis=1)
        _bury(dead, X=X[idx], y=y[idx], L=L[idx], logw=logw, cl=cid,
              logX=mx + np.log(np.sum(np.exp(after - mx[:, None]), axis=1)))

    def logZ_live():
        return _logsumexp([logXc[q] + _logsumexp(L[cl == q]) - np.log(np.count_nonzero(cl == q)) for q in open_ids])

    if nprior > nlive:
        rem, keep, _ = _split(L, nprior - nlive, minus_inf_value)
        kill(rem)
        X, y, L, cl = X[keep], y[keep], L[keep], cl[keep]
    gen = 0
    while _goes_on(dead, logZ_live(), precision_criterion, ncalls, max_ncalls, gen):
        rem, keep, thr = _split(L, k_gen, minus_inf_value)
        kill(rem)
        Xs, ys = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
        Ls, cls = L[keep], cl[keep]
        Us = (Xs - lo) / (hi - lo)
        # re-cluster every open cluster's survivors on their own; an emptied cluster is closed (its volume dropped),
        # a split one is closed and its children share its volume in proportion to their live counts
        still = []
        for q in open_ids:
            mem = np.flatnonzero(cls == q)
            if len(mem) == 0:
                continue
            lab, nc, ms = _clusters_of(dev, lo, hi, np.ascontiguousarray(Xs[mem]), k_max)
            device_ms += ms
            if nc == 1:
                still.append(q)
                continue
            counts = np.bincount(lab)
            for part in range(nc):
                parent.append(q)
                logXc.append(logXc[q] + np.log(counts[part] / len(mem)))
                cls[mem[lab == part]] = len(parent) - 1
                still.append(len(parent) - 1)
        open_ids = still
        ids = np.array(open_ids, dtype=np.int64)
        pos = np.empty(len(parent), np.int64)
        pos[ids] = np.arange(len(ids))
        labels = pos[cls].astype(np.int32)
        cum_p = cluster_probabilities([logXc[q] for q in open_ids])
        # every cluster walks with the matrix of its own survivors, also once kills have left it fewer than d + 1 (the
        # ridge of cholesky_ridged keeps it positive definite): a matrix fitted to more points would span the gap to
        # another mode, and a chain that jumps across is charged to the wrong cluster (profiles/nested_volumes.md)
        W = np.stack([whitening(Us[labels == i]) for i in range(len(ids))])
        n_clusters.append(len(ids))
        Xn, yn, cnt, _, _, ms = _generation(dev, None, lo, hi, Xs, ys, thr, W, seed, gen, k_gen, num_repeats,
                                            labels=labels, cum_p=cum_p)
        device_ms += ms
        ncalls += int(np.sum(cnt))
        X = np.concatenate([Xs, Xn])
        y = np.concatenate([ys, yn])
        L = np.concatenate([Ls, _logL(yn, minus_inf_value)])
        cl = np.concatenate([cls, ids[chain_clusters(seed, gen, k_gen, cum_p)]])
        gen += 1
    # the final live points: volume X_q / n_q each
    nq = np.bincount(cl, minlength=len(parent)).astype(float)
    res, all_L, all_logw = _finish(dead, X, y, L, L + np.array(logXc)[cl] - np.log(nq[cl]), nlive, ncalls, gen, device_ms,
                                   n_clusters)
    all_cl = np.concatenate(dead["cl"] + [cl])
    return dict(res, cluster=np.ascontiguousarray(all_cl[np.isfinite(all_L)]),
                cluster_logZ=np.array([_logsumexp(all_logw[all_cl == q]) for q in range(len(parent))]),
                cluster_parent=np.array(parent, dtype=np.int64))
