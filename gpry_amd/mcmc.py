"""Metropolis MCMC of the surrogate's posterior mean, with the chains run on the device.

The reference samples the surrogate with Cobaya's MCMC (gpry/mc.py:173-327; GaussianKL's MC fallback at temperature 2,
gpry/convergence.py:430-476; SmallChainProposer, gpry/proposal.py:359-443), which calls ``gpr.predict`` once per step.
Here whole batches of steps of many chains run in one HIP kernel (``gpry_amd/csrc/mcmc.hip``).  This module keeps the
rest: the start points, the adaptation of the proposal, the convergence test, the burn-in and the weights.  It talks to
the device through one call, so any object with the same method can stand in for it (the CPU tests use a numpy one):

``dev.mcmc_chains(lo, hi, X0, y0, Lp, T, minus_inf_value, seed, batch, nsteps, thin)
    -> {"X": (nchains, nsteps // thin, d), "y": (nchains, nsteps // thin), "X_last", "y_last", "naccept", "ncalls",
        "device_ms"}``

The algorithm, step by step:

* The chains work in the unit cube u = (x - lo) / (hi - lo); the prior is uniform on the box.  The target is
  exp(y / T).
* Starts: ``nchains`` training points drawn with replacement, with probability ∝ exp((y - y_max) / T), from an rng
  seeded with ``seed`` (the reference starts chain r at the (r+1)-th best point, gpry/mc.py:140-146; drawing disperses
  the starts, which the multi-chain test of convergence needs).  Their y is evaluated on the device.
* Adaptation: the first proposal is ``covmat`` (raw coordinates) or the exp(y - y_max)-weighted covariance of the
  training set; then ``learn_batches`` batches of ``learn_every`` steps, after each of which the covariance is
  re-estimated from the second half of that batch's states, pooled over the chains.  Every proposal factor is the
  Cholesky factor of the covariance (``nested.cholesky_ridged``) times 2.38 / sqrt(d).  Then the proposal is frozen, and
  everything sampled after is a homogeneous Markov chain.
* Sampling: batches of ``batch_steps`` steps, a state recorded every ``thin`` steps.  After each batch the first ``skip``
  fraction of every chain's records is dropped, every chain is split in halves, and R - 1 is computed over those
  2 nchains sequences (``rminus1``).  Stop when R - 1 < ``Rminus1_stop``, or, not converged, at the end of a batch once
  ``max_ncalls`` evaluations or ``max_batches`` batches are reached.
* Output: the records of the sampling phase without the ``skip`` fraction of each chain, rows of finite y only.  With
  T != 1 and ``reset_temperature``, the weights are ∝ exp(y - y / T) (Cobaya's ``reset_temperature``), else equal.
"""
from collections import namedtuple
from time import time

import numpy as np

from gpry_amd.nested import cholesky_ridged

MCMCResult = namedtuple("MCMCResult", ["X", "y", "w", "Rminus1", "acceptance", "ncalls", "batches", "covmat",
                                       "converged", "device_s", "wall_s"])
MCMCResult.__doc__ = """Output of ``run_mcmc``.  X, y, w: the sample (w sums to 1); Rminus1: R - 1 after each sampling
batch; acceptance: accepted / proposed steps of the sampling phase; ncalls: evaluations of the surrogate, adaptation and
starts included; batches: sampling batches; covmat: the learned covariance of the frozen proposal, raw coordinates,
without the 2.38 / sqrt(d) scale; converged: R - 1 reached ``Rminus1_stop``; device_s / wall_s: time in the device calls
/ in the whole run."""

# Defaults measured on the bench's fitted model (N = 4096, d = 16; profiles/mcmc.md)
DEFAULT_NCHAINS = 256
DEFAULT_LEARN_EVERY = 100
DEFAULT_LEARN_BATCHES = 4
DEFAULT_BATCH_STEPS = 1000
DEFAULT_MAX_BATCHES = 1000
PROPOSAL_SCALE = 2.38


def rminus1(seqs):
    """Multivariate R - 1 of m sequences (m, n, d) in Cobaya's form: the largest eigenvalue of W^-1 B, W the mean of the
    sequences' covariances, B the covariance of their means (both with ddof = 1)."""
    seqs = np.asarray(seqs, dtype=float)
    m, n, d = seqs.shape
    if m < 2 or n < 2:
        return np.inf
    means = seqs.mean(axis=1)
    dev = seqs - means[:, None, :]
    return _rminus1_of(means, np.einsum("mni,mnj->mij", dev, dev) / (n - 1))


def _rminus1_of(means, covs):
    W = covs.mean(axis=0)
    B = np.atleast_2d(np.cov(means, rowvar=False, ddof=1))
    try:
        L = np.linalg.cholesky(W)
    except np.linalg.LinAlgError:
        return np.inf
    Li = np.linalg.inv(L)
    return float(np.max(np.abs(np.linalg.eigvalsh(Li @ B @ Li.T))))


class _Records:
    """The sampling phase's records, batch by batch, with each batch's per-chain sums of x and x x^T (about a fixed
    shift), so that R - 1 of the split chains after the burn-in costs O(batches m d^2) plus the two batches the window
    boundaries cut, instead of a pass over every record after every batch."""

    def __init__(self):
        self.X, self.y, self.s1, self.s2, self.start = [], [], [], [], [0]
        self.shift = None

    def add(self, X, y):
        if self.shift is None:
            self.shift = X.reshape(-1, X.shape[2]).mean(axis=0)
        Xc = X - self.shift
        self.X.append(X)
        self.y.append(y)
        self.s1.append(Xc.sum(axis=1))
        self.s2.append(np.einsum("mni,mnj->mij", Xc, Xc))
        self.start.append(self.start[-1] + X.shape[1])

    @property
    def n(self):
        return self.start[-1]

    def _sums(self, a, e):
        """Per-chain sums of x and x x^T (shifted) over the records a .. e - 1."""
        m, d = self.X[0].shape[0], self.X[0].shape[2]
        s1, s2 = np.zeros((m, d)), np.zeros((m, d, d))
        for k, X in enumerate(self.X):
            lo, hi = max(a, self.start[k]), min(e, self.start[k + 1])
            if lo >= hi:
                continue
            if lo == self.start[k] and hi == self.start[k + 1]:
                s1 += self.s1[k]
                s2 += self.s2[k]
            else:
                Xc = X[:, lo - self.start[k]:hi - self.start[k]] - self.shift
                s1 += Xc.sum(axis=1)
                s2 += np.einsum("mni,mnj->mij", Xc, Xc)
        return s1, s2

    def rminus1(self, first):
        """R - 1 of the records first .. n - 1 of every chain, each split in halves."""
        h = (self.n - first) // 2
        if h < 2:
            return np.inf
        means, covs = [], []
        for a in (first, first + h):
            s1, s2 = self._sums(a, a + h)
            mu = s1 / h
            means.append(mu)
            covs.append((s2 - h * np.einsum("mi,mj->mij", mu, mu)) / (h - 1))
        return _rminus1_of(np.concatenate(means), np.concatenate(covs))

    def kept(self, first):
        return np.concatenate(self.X, axis=1)[:, first:], np.concatenate(self.y, axis=1)[:, first:]


def _weighted_cov(X, y, T=1.0):
    w = np.exp((y - np.max(y)) / T)
    w /= w.sum()
    m = w @ X
    return (X - m).T @ ((X - m) * w[:, None])


def _starts(X0, y0, lo, hi, T, minus_inf_value, nchains, seed):
    """The start rule: the usable training points (finite y above ``minus_inf_value``, inside the box) and ``nchains`` of
    them drawn with replacement with probability ∝ exp((y - y_max) / T) from an rng seeded with ``seed``: ``(Xt, yt, Xs,
    ys)``, ys all NaN (the device evaluates the starts)."""
    ok = np.isfinite(y0) & (y0 > minus_inf_value) & np.all((X0 >= lo) & (X0 <= hi), axis=1)
    if not ok.any():
        raise ValueError("no training point with a finite y inside the bounds to start a chain from")
    Xt, yt = X0[ok], y0[ok]
    rng = np.random.default_rng(seed)
    p = np.exp((yt - np.max(yt)) / T)
    Xs = np.ascontiguousarray(Xt[rng.choice(len(yt), size=nchains, p=p / p.sum())])
    return Xt, yt, Xs, np.full(nchains, np.nan)


def _temperature_weights(y, T, reset_temperature):
    """Normalised weights of a sample of exp(y / T): ∝ exp(y - y / T) with ``reset_temperature`` and T != 1, else equal."""
    if T != 1.0 and reset_temperature and len(y):
        logw = y - y / T
        w = np.exp(logw - np.max(logw))
    else:
        w = np.ones(len(y))
    return w / w.sum() if len(w) else w


def run_mcmc(dev, bounds, seed, nchains, X0, y0, temperature=1.0, covmat=None, learn_every=DEFAULT_LEARN_EVERY,
             learn_batches=DEFAULT_LEARN_BATCHES, batch_steps=DEFAULT_BATCH_STEPS, thin=None, Rminus1_stop=0.01,
             max_ncalls=None, max_batches=DEFAULT_MAX_BATCHES, skip=0.33, reset_temperature=True,
             minus_inf_value=-np.inf):
    """Metropolis run of the surrogate on ``dev``; see the module's docstring.  X0, y0: the training set the starts are
    drawn from.  ``thin`` (default d): steps between records of the sampling phase.  Returns an ``MCMCResult``."""
    t_start = time()
    bounds = np.asarray(bounds, dtype=float)
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    span = hi - lo
    d = len(lo)
    nchains, seed, T = int(nchains), int(seed), float(temperature)
    thin = d if thin is None else int(thin)
    learn_every, learn_batches, batch_steps = int(learn_every), int(learn_batches), int(batch_steps)
    if nchains < 1:
        raise ValueError(f"nchains = {nchains}: at least one chain is needed")
    if not (np.isfinite(T) and T > 0):
        raise ValueError(f"temperature = {T} must be positive and finite")
    if thin < 1 or batch_steps < thin or learn_batches < 0 or (learn_batches > 0 and learn_every < 2):
        raise ValueError(f"thin = {thin}, batch_steps = {batch_steps}, learn_every = {learn_every}, "
                         f"learn_batches = {learn_batches}: need 1 <= thin <= batch_steps and learn_every >= 2")
    if not 0.0 <= skip < 1.0:
        raise ValueError(f"skip = {skip} must lie in [0, 1)")
    if int(max_batches) < 1:
        raise ValueError(f"max_batches = {max_batches}: at least one sampling batch is needed")
    X0, y0 = np.atleast_2d(np.asarray(X0, dtype=float)), np.asarray(y0, dtype=float).ravel()
    if X0.shape != (len(y0), d):
        raise ValueError(f"X0 {X0.shape} and y0 {y0.shape} do not form a training set of dimension {d}")
    Xt, yt, Xs, ys = _starts(X0, y0, lo, hi, T, minus_inf_value, nchains, seed)
    # ---- first proposal, unit-cube coordinates
    C_u = (np.asarray(covmat, dtype=float) if covmat is not None else _weighted_cov(Xt, yt)) / np.outer(span, span)
    scale = PROPOSAL_SCALE / np.sqrt(d)
    Lp = scale * cholesky_ridged(C_u)
    device_ms, ncalls, batch = 0.0, 0, 0

    def step(nsteps, thin_):
        nonlocal Xs, ys, device_ms, ncalls, batch
        out = dev.mcmc_chains(lo, hi, Xs, ys, Lp, T, minus_inf_value, seed, batch, nsteps, thin_)
        batch += 1
        device_ms += out["device_ms"]
        ncalls += int(np.sum(out["ncalls"]))
        Xs, ys = out["X_last"], out["y_last"]
        return out

    # ---- adaptation
    for _ in range(learn_batches):
        out = step(learn_every, 1)
        half = out["X"][:, learn_every // 2:].reshape(-1, d)
        C_u = np.atleast_2d(np.cov((half - lo) / span, rowvar=False, ddof=0))
        Lp = scale * cholesky_ridged(C_u)
    # ---- sampling with the frozen proposal
    rec, Rm = _Records(), []
    nacc, nprop, nbatch, converged = 0, 0, 0, False
    while True:
        out = step(batch_steps, thin)
        nbatch += 1
        nacc += int(np.sum(out["naccept"]))
        nprop += nchains * batch_steps
        rec.add(out["X"], out["y"])
        first = int(skip * rec.n)
        Rm.append(rec.rminus1(first))
        if Rm[-1] < Rminus1_stop:
            converged = True
            break
        if (max_ncalls is not None and ncalls >= max_ncalls) or nbatch >= int(max_batches):
            break
    X, y = rec.kept(first)
    X, y = X.reshape(-1, d), y.ravel()
    fin = np.isfinite(y) & (y > minus_inf_value)
    X, y = np.ascontiguousarray(X[fin]), np.ascontiguousarray(y[fin])
    w = _temperature_weights(y, T, reset_temperature)
    return MCMCResult(X=X, y=y, w=w, Rminus1=np.array(Rm), acceptance=nacc / max(nprop, 1), ncalls=ncalls,
                      batches=nbatch, covmat=C_u * np.outer(span, span), converged=converged,
                      device_s=device_ms / 1e3, wall_s=time() - t_start)
