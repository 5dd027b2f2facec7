"""Tempered Metropolis ladders (parallel tempering) of the surrogate's posterior mean, with the ladders run on the device.

The chains of ``gpry_amd/mcmc.py`` cannot change modes: on a surrogate with separated modes every chain stays where its
start was drawn, R - 1 never falls and the mode masses are those of the start draw.  Here every cold chain is the lowest
rung of a ladder of chains at rising temperatures T[0] < T[1] < ...; rung r samples exp(y / T[r]), the hot rungs cross
between the modes, and swaps of the states of adjacent rungs carry the crossings down to the cold one (Swendsen & Wang
1986; Geyer 1991).  One workgroup runs one ladder and evaluates the proposals of all its rungs in one pass over the
training rows (``gpry_amd/csrc/mcmc_ladders.hip``).  This module keeps the rest and talks to the device through one call,
so any object with the same method can stand in for it (the CPU tests use a numpy one, tests/tools/tempering_numpy.py):

``dev.mcmc_ladders(lo, hi, X0, y0, nrungs, Lp, T, minus_inf_value, seed, batch, nsteps, thin, swap_every)
    -> the dict of ``mcmc_chains`` over the nladders * nrungs chains (chain a * nrungs + r: rung r of ladder a), plus
       "nswap_try", "nswap_acc": (nladders, nrungs - 1)``

The algorithm, step by step:

* Ladder: ``temperatures`` as given (T[0] is the target's temperature), or ``rungs`` levels from ``temperature`` with the
  ratio rho between neighbours: rho = (T_max / temperature)^(1 / (rungs - 1)) with ``T_max``, else rho = 1 + sqrt(8 / d).
  For Gaussian rungs that ratio gave a swap acceptance of 0.50 / 0.41 / 0.35 / 0.29 / 0.26 at d = 2 / 4 / 8 / 16 / 32 in a
  numpy model; it is provisional (profiles/mcmc_tempering.md has what the device measured).
* Starts: the rule of ``run_mcmc`` (``mcmc._starts``), one draw of nladders * rungs training points at the target's
  temperature; their y is evaluated on the device.
* A step (the device's part): every rung makes the Metropolis step of ``gpry_mcmc_chains`` with its own proposal and
  temperature.  After every ``swap_every``-th step a swap round: round q tries the pairs (r, r + 1) with r = q (mod 2);
  a pair whose y are both usable exchanges its states iff log(1 - us) < (1 / T[r] - 1 / T[r + 1]) (y_{r+1} - y_r).
* Adaptation, swaps off: rung r's first proposal is ``covmat`` (or the exp(y - y_max)-weighted covariance of the training
  set) times T[r] / T[0]; then ``learn_batches`` batches of ``learn_every`` steps, after each of which rung r's covariance
  becomes the mean over the ladders of each chain's own covariance over the second half of the batch -- the W of R - 1,
  not the pooled covariance, which separate modes would inflate to the distance between them.  Every proposal factor is
  the Cholesky factor (``nested.cholesky_ridged``) times 2.38 / sqrt(d).  Then the proposals are frozen.
* Sampling, swaps on: batches of ``batch_steps`` steps, the state of every rung recorded every ``thin`` steps.  R - 1 is
  computed over the split sequences of the ladders' rungs 0 (``mcmc._Records``), with the stopping rules of ``run_mcmc``;
  ``max_ncalls`` counts the evaluations of every rung.
* Output: the records of rung 0 without the ``skip`` fraction, rows of finite y only, with the weights
  ``mcmc._temperature_weights(y, T[0], reset_temperature)``.
"""
from collections import namedtuple
from time import time

import numpy as np

from gpry_amd.mcmc import MCMCResult, PROPOSAL_SCALE, _Records, _starts, _temperature_weights, _weighted_cov
from gpry_amd.nested import cholesky_ridged

TemperedResult = namedtuple("TemperedResult", MCMCResult._fields + ("temperatures", "swap_acceptance",
                                                                    "acceptance_per_rung"))
TemperedResult.__doc__ = """Output of ``run_tempered``.  The fields of ``MCMCResult`` for rung 0 (ncalls: evaluations of
every rung, adaptation and starts included; acceptance: rung 0's; covmat: rung 0's frozen covariance), and temperatures:
the ladder; swap_acceptance: accepted / tried swaps of every adjacent pair over the sampling phase (NaN: none tried);
acceptance_per_rung: accepted / proposed Metropolis steps of every rung over the sampling phase."""

DEFAULT_NLADDERS = 64
DEFAULT_RUNGS = 6
DEFAULT_SWAP_EVERY = 5
DEFAULT_LEARN_EVERY = 100
DEFAULT_LEARN_BATCHES = 4
DEFAULT_BATCH_STEPS = 1000
DEFAULT_MAX_BATCHES = 1000
MAX_RUNGS = 8


def ladder(d, temperature=1.0, rungs=DEFAULT_RUNGS, T_max=None, temperatures=None):
    """The temperatures of a ladder: ``temperatures`` as given (strictly increasing, positive, finite), or ``rungs``
    levels from ``temperature`` in geometric progression, up to ``T_max`` or with the ratio 1 + sqrt(8 / d)."""
    if temperatures is not None:
        T = np.array(temperatures, dtype=float).ravel()
        if len(T) < 1 or not np.all(np.isfinite(T) & (T > 0)) or np.any(np.diff(T) <= 0):
            raise ValueError(f"temperatures = {temperatures} must be positive, finite and strictly increasing")
    else:
        rungs, T0 = int(rungs), float(temperature)
        if rungs < 1:
            raise ValueError(f"rungs = {rungs}: at least one rung is needed")
        if not (np.isfinite(T0) and T0 > 0):
            raise ValueError(f"temperature = {T0} must be positive and finite")
        if T_max is None:
            rho = 1.0 + np.sqrt(8.0 / d)
        else:
            if rungs < 2 or not (np.isfinite(T_max) and T_max > T0):
                raise ValueError(f"T_max = {T_max} needs rungs >= 2 and a finite T_max > temperature = {T0}")
            rho = (float(T_max) / T0) ** (1.0 / (rungs - 1))
        T = T0 * rho ** np.arange(rungs)
    if len(T) > MAX_RUNGS:
        raise ValueError(f"{len(T)} rungs: a ladder has at most {MAX_RUNGS}")
    return T


def _within_chain_cov(U):
    """The mean over the chains of each chain's own covariance (ddof = 1): U (m, n, d) -> (d, d)."""
    dev = U - U.mean(axis=1, keepdims=True)
    return np.einsum("mni,mnj->ij", dev, dev) / (U.shape[0] * (U.shape[1] - 1))


def run_tempered(dev, bounds, seed, nladders, X0, y0, temperature=1.0, rungs=DEFAULT_RUNGS, T_max=None, temperatures=None,
                 swap_every=DEFAULT_SWAP_EVERY, covmat=None, learn_every=DEFAULT_LEARN_EVERY,
                 learn_batches=DEFAULT_LEARN_BATCHES, batch_steps=DEFAULT_BATCH_STEPS, thin=None, Rminus1_stop=0.01,
                 max_ncalls=None, max_batches=DEFAULT_MAX_BATCHES, skip=0.33, reset_temperature=True,
                 minus_inf_value=-np.inf):
    """Tempered run of the surrogate on ``dev``; see the module's docstring.  X0, y0: the training set the starts are
    drawn from.  ``thin`` (default d): steps between records of the sampling phase.  Returns a ``TemperedResult``."""
    t_start = time()
    bounds = np.asarray(bounds, dtype=float)
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    span = hi - lo
    d = len(lo)
    nladders, seed, swap_every = int(nladders), int(seed), int(swap_every)
    thin = d if thin is None else int(thin)
    learn_every, learn_batches, batch_steps = int(learn_every), int(learn_batches), int(batch_steps)
    if nladders < 1:
        raise ValueError(f"nladders = {nladders}: at least one ladder is needed")
    T = ladder(d, temperature, rungs, T_max, temperatures)
    R = len(T)
    if swap_every < 0:
        raise ValueError(f"swap_every = {swap_every} must not be negative")
    if thin < 1 or batch_steps < thin or learn_batches < 0 or (learn_batches > 0 and learn_every < 4):
        raise ValueError(f"thin = {thin}, batch_steps = {batch_steps}, learn_every = {learn_every}, "
                         f"learn_batches = {learn_batches}: need 1 <= thin <= batch_steps and learn_every >= 4")
    if not 0.0 <= skip < 1.0:
        raise ValueError(f"skip = {skip} must lie in [0, 1)")
    if int(max_batches) < 1:
        raise ValueError(f"max_batches = {max_batches}: at least one sampling batch is needed")
    X0, y0 = np.atleast_2d(np.asarray(X0, dtype=float)), np.asarray(y0, dtype=float).ravel()
    if X0.shape != (len(y0), d):
        raise ValueError(f"X0 {X0.shape} and y0 {y0.shape} do not form a training set of dimension {d}")
    Xt, yt, Xs, ys = _starts(X0, y0, lo, hi, T[0], minus_inf_value, nladders * R, seed)
    # ---- first proposals, unit-cube coordinates
    C0 = (np.asarray(covmat, dtype=float) if covmat is not None else _weighted_cov(Xt, yt)) / np.outer(span, span)
    scale = PROPOSAL_SCALE / np.sqrt(d)
    C_u = np.array([C0 * (T[r] / T[0]) for r in range(R)])
    Lp = np.array([scale * cholesky_ridged(C) for C in C_u])
    device_ms, ncalls, batch = 0.0, 0, 0

    def step(nsteps, thin_, swaps):
        nonlocal Xs, ys, device_ms, ncalls, batch
        out = dev.mcmc_ladders(lo, hi, Xs, ys, R, Lp, T, minus_inf_value, seed, batch, nsteps, thin_, swaps)
        batch += 1
        device_ms += out["device_ms"]
        ncalls += int(np.sum(out["ncalls"]))
        Xs, ys = out["X_last"], out["y_last"]
        return out

    # ---- adaptation, swaps off
    for _ in range(learn_batches):
        out = step(learn_every, 1, 0)
        U = ((out["X"] - lo) / span).reshape(nladders, R, learn_every, d)[:, :, learn_every // 2:]
        C_u = np.array([_within_chain_cov(U[:, r]) for r in range(R)])
        Lp = np.array([scale * cholesky_ridged(C) for C in C_u])
    # ---- sampling with the frozen proposals, swaps on
    rec, Rm = _Records(), []
    nacc, nprop, nbatch, converged = np.zeros(R, np.int64), 0, 0, False
    ntry, nsw = np.zeros(max(R - 1, 0), np.int64), np.zeros(max(R - 1, 0), np.int64)
    while True:
        out = step(batch_steps, thin, swap_every)
        nbatch += 1
        nacc += np.asarray(out["naccept"]).reshape(nladders, R).sum(axis=0)
        nprop += nladders * batch_steps
        ntry += np.asarray(out["nswap_try"]).reshape(nladders, R - 1).sum(axis=0)
        nsw += np.asarray(out["nswap_acc"]).reshape(nladders, R - 1).sum(axis=0)
        nrec = out["X"].shape[1]
        rec.add(out["X"].reshape(nladders, R, nrec, d)[:, 0], out["y"].reshape(nladders, R, nrec)[:, 0])
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
    w = _temperature_weights(y, float(T[0]), reset_temperature)
    with np.errstate(invalid="ignore", divide="ignore"):
        swap_acc = np.where(ntry > 0, nsw / np.maximum(ntry, 1), np.nan)
    per_rung = nacc / max(nprop, 1)
    return TemperedResult(X=X, y=y, w=w, Rminus1=np.array(Rm), acceptance=float(per_rung[0]), ncalls=ncalls,
                          batches=nbatch, covmat=C_u[0] * np.outer(span, span), converged=converged,
                          device_s=device_ms / 1e3, wall_s=time() - t_start, temperatures=T, swap_acceptance=swap_acc,
                          acceptance_per_rung=per_rung)
