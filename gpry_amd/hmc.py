"""Hamiltonian Monte Carlo of the surrogate's posterior mean, with the chains run on the device.

A second sampler for what ``gpry_amd/mcmc.py`` samples (the surrogate's final sample, gpry/mc.py:173-327; GaussianKL's MC
fallback, gpry/convergence.py:430-476; SmallChainProposer, gpry/proposal.py:359-443).  A random walk pays roughly d^2
evaluations per independent point; a leapfrog trajectory driven by the gradient of the mean pays roughly d^(5/4), and the
gradient costs about one evaluation (the same pass over the training rows).  Whole batches of trajectories of many chains
run in one HIP kernel (``gpry_amd/csrc/hmc.hip``), the gradient evaluated inside it.  This module keeps the rest and
talks to the device through one call, so any object with the same method can stand in for it (the CPU tests use a numpy
one, tests/tools/hmc_numpy.py):

``dev.hmc_chains(lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin)
    -> {"X": (nchains, nsteps // thin, d), "y": (nchains, nsteps // thin), "X_last", "y_last", "naccept", "ncalls",
        "ngrad", "device_ms"}``

(with ``reflect=True, max_reflect=`` as keywords when reflection is on, and then ``"nreflect"`` in the result).

The algorithm, step by step:

* The chains work in the unit cube u = (x - lo) / (hi - lo); the prior is uniform on the box.  The target is
  exp(y / T).
* Starts: the rule of ``run_mcmc`` (``mcmc._starts``): ``nchains`` training points drawn with probability
  ∝ exp((y - y_max) / T) from an rng seeded with ``seed``; their y is evaluated on the device.
* A trajectory (the device's part): momentum p ~ N(0, I); a half kick p += (eps_s / 2) Lp^T g(u) / T, then ``nleap``
  times a drift u += eps_s Lp p and a kick (the last a half one), with g the gradient of the unclipped, ungated mean in
  unit-cube coordinates and eps_s = eps (0.8 + 0.4 u), u uniform, drawn per trajectory.  A drift that leaves the box
  rejects the trajectory at once.  The end point is accepted iff its y' (``gpr.predict``, clip and gates included) is
  finite, above ``minus_inf_value`` and log(1 - ua) < (y' - y) / T - (|p'|^2 - |p|^2) / 2.
* Reflection (``reflect=True``, off by default): the drift becomes a billiard flow of duration eps_s inside the unit
  cube.  Where a coordinate's wall is hit before the time is up, the chain moves to the wall, its momentum is reflected
  about the wall's normal in the whitened coordinates q = Lp^-1 u (p -= 2 (r . p) / (r . r) r, r the wall coordinate's row
  of Lp), and the drift goes on with what time is left; a single drift that would need more than ``max_reflect``
  reflections rejects the trajectory as a box exit does without reflection.  Reflection keeps |p|^2 and the flow is
  volume-preserving and reversible, so the acceptance rule is unchanged and the chain stays exact (Neal 2011, section
  5.5.1.5).  No trajectory is then lost to the walls, and the step size answers to the energy error alone.
* Adaptation: the first mass-matrix inverse is ``covmat`` (raw coordinates) or the exp(y - y_max)-weighted covariance of
  the training set, in unit-cube coordinates; ``Lp`` is its Cholesky factor (``nested.cholesky_ridged``), no scale.
  Then ``learn_batches`` batches of ``learn_every`` trajectories.  After each, the covariance is re-estimated from the
  second half of that batch's states, pooled over the chains; the step size moves towards the target acceptance,
  eps <- eps clip(exp(1.5 (acc - accept_target)), 0.5, 2), acc the batch's accepted / proposed trajectories; and
  nleap = clip(ceil(1.57 / eps), 4, 64), a quarter period of a whitened Gaussian.  Then everything is frozen, and what
  is sampled after is a homogeneous Markov chain.
* Sampling: batches of ``batch_steps`` trajectories, a state recorded every ``thin``.  The convergence test is
  ``run_mcmc``'s (``mcmc._Records``): the first ``skip`` fraction of every chain's records dropped, every chain split
  in halves, R - 1 over those 2 nchains sequences.  Stop when R - 1 < ``Rminus1_stop``, or, not converged, at the end of
  a batch once ``max_ncalls`` evaluations (mean + gradient) or ``max_batches`` batches are reached.
* Output: as ``run_mcmc``: the records of the sampling phase without the ``skip`` fraction, rows of finite y only, with
  the temperature weights of ``mcmc._temperature_weights``.
"""
from collections import namedtuple
from time import time

import numpy as np

from gpry_amd.mcmc import MCMCResult, _Records, _starts, _temperature_weights, _weighted_cov
from gpry_amd.nested import cholesky_ridged

HMCResult = namedtuple("HMCResult", MCMCResult._fields + ("eps", "nleap", "ngrad", "nreflect"))
HMCResult.__doc__ = """Output of ``run_hmc``.  The fields of ``MCMCResult`` (ncalls: evaluations of the mean, adaptation
and starts included; acceptance: accepted / proposed trajectories of the sampling phase; covmat: the frozen mass-matrix
inverse, raw coordinates), and eps, nleap: the frozen step size and leapfrog steps per trajectory; ngrad: the gradient
evaluations, each about the cost of one evaluation of the mean; nreflect: the reflections at the walls over the whole run
(0 without ``reflect``)."""

DEFAULT_NCHAINS = 256
DEFAULT_LEARN_EVERY = 40
DEFAULT_LEARN_BATCHES = 6
DEFAULT_BATCH_STEPS = 50
DEFAULT_MAX_BATCHES = 1000
DEFAULT_ACCEPT_TARGET = 0.8
NLEAP_MIN, NLEAP_MAX = 4, 64
QUARTER_PERIOD = 1.57


def leapfrog_steps(eps):
    """nleap of a step size: a quarter period of a whitened Gaussian, clipped to [4, 64]."""
    return int(np.clip(np.ceil(QUARTER_PERIOD / eps), NLEAP_MIN, NLEAP_MAX))


def run_hmc(dev, bounds, seed, nchains, X0, y0, temperature=1.0, covmat=None, eps=None, accept_target=DEFAULT_ACCEPT_TARGET,
            learn_every=DEFAULT_LEARN_EVERY, learn_batches=DEFAULT_LEARN_BATCHES, batch_steps=DEFAULT_BATCH_STEPS, thin=1,
            Rminus1_stop=0.01, max_ncalls=None, max_batches=DEFAULT_MAX_BATCHES, skip=0.33, reset_temperature=True,
            minus_inf_value=-np.inf, reflect=False, max_reflect=64):
    """HMC run of the surrogate on ``dev``; see the module's docstring.  X0, y0: the training set the starts are drawn
    from.  ``eps``: the first step size (default d^(-1/4)).  ``reflect``: trajectories reflect at the walls of the box,
    at most ``max_reflect`` times per drift.  Returns an ``HMCResult``."""
    t_start = time()
    bounds = np.asarray(bounds, dtype=float)
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    span = hi - lo
    d = len(lo)
    nchains, seed, T, thin = int(nchains), int(seed), float(temperature), int(thin)
    learn_every, learn_batches, batch_steps = int(learn_every), int(learn_batches), int(batch_steps)
    eps = float(d) ** -0.25 if eps is None else float(eps)
    if nchains < 1:
        raise ValueError(f"nchains = {nchains}: at least one chain is needed")
    if not (np.isfinite(T) and T > 0):
        raise ValueError(f"temperature = {T} must be positive and finite")
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError(f"eps = {eps} must be positive and finite")
    if not 0.0 < accept_target < 1.0:
        raise ValueError(f"accept_target = {accept_target} must lie in (0, 1)")
    if thin < 1 or batch_steps < thin or learn_batches < 0 or (learn_batches > 0 and learn_every < 2):
        raise ValueError(f"thin = {thin}, batch_steps = {batch_steps}, learn_every = {learn_every}, "
                         f"learn_batches = {learn_batches}: need 1 <= thin <= batch_steps and learn_every >= 2")
    if not 0.0 <= skip < 1.0:
        raise ValueError(f"skip = {skip} must lie in [0, 1)")
    reflect, max_reflect = bool(reflect), int(max_reflect)
    if reflect and not 1 <= max_reflect <= 1024:
        raise ValueError(f"max_reflect = {max_reflect} must lie in 1 .. 1024")
    if int(max_batches) < 1:
        raise ValueError(f"max_batches = {max_batches}: at least one sampling batch is needed")
    X0, y0 = np.atleast_2d(np.asarray(X0, dtype=float)), np.asarray(y0, dtype=float).ravel()
    if X0.shape != (len(y0), d):
        raise ValueError(f"X0 {X0.shape} and y0 {y0.shape} do not form a training set of dimension {d}")
    Xt, yt, Xs, ys = _starts(X0, y0, lo, hi, T, minus_inf_value, nchains, seed)
    # ---- first mass-matrix inverse, unit-cube coordinates
    C_u = (np.asarray(covmat, dtype=float) if covmat is not None else _weighted_cov(Xt, yt)) / np.outer(span, span)
    Lp = cholesky_ridged(C_u)
    nleap = leapfrog_steps(eps)
    device_ms, ncalls, ngrad, nreflect, batch = 0.0, 0, 0, 0, 0
    own = dict(reflect=True, max_reflect=max_reflect) if reflect else {}

    def step(nsteps, thin_):
        nonlocal Xs, ys, device_ms, ncalls, ngrad, nreflect, batch
        out = dev.hmc_chains(lo, hi, Xs, ys, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin_, **own)
        batch += 1
        device_ms += out["device_ms"]
        ncalls += int(np.sum(out["ncalls"]))
        ngrad += int(np.sum(out["ngrad"]))
        if reflect:
            nreflect += int(np.sum(out["nreflect"]))
        Xs, ys = out["X_last"], out["y_last"]
        return out

    # ---- adaptation
    for _ in range(learn_batches):
        out = step(learn_every, 1)
        half = out["X"][:, learn_every // 2:].reshape(-1, d)
        C_u = np.atleast_2d(np.cov((half - lo) / span, rowvar=False, ddof=0))
        Lp = cholesky_ridged(C_u)
        acc = float(np.sum(out["naccept"])) / (nchains * learn_every)
        eps *= float(np.clip(np.exp(1.5 * (acc - accept_target)), 0.5, 2.0))
        nleap = leapfrog_steps(eps)
    # ---- sampling with everything frozen
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
        if (max_ncalls is not None and ncalls + ngrad >= max_ncalls) or nbatch >= int(max_batches):
            break
    X, y = rec.kept(first)
    X, y = X.reshape(-1, d), y.ravel()
    fin = np.isfinite(y) & (y > minus_inf_value)
    X, y = np.ascontiguousarray(X[fin]), np.ascontiguousarray(y[fin])
    w = _temperature_weights(y, T, reset_temperature)
    return HMCResult(X=X, y=y, w=w, Rminus1=np.array(Rm), acceptance=nacc / max(nprop, 1), ncalls=ncalls,
                     batches=nbatch, covmat=C_u * np.outer(span, span), converged=converged,
                     device_s=device_ms / 1e3, wall_s=time() - t_start, eps=eps, nleap=nleap, ngrad=ngrad,
                     nreflect=nreflect)
