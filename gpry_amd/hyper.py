"""How well the data determine the hyper-parameters: the Laplace approximation of the marginal likelihood in theta.

``hyper_laplace(gpr)`` evaluates the log marginal likelihood, its gradient and its Hessian at theta in one device call
(``gpry_lml_hessian``, closed form) and reads from them which entries the data pin and which are sloppy, how they are
correlated, which are held by a bound, and the Laplace evidence of the kernel family.  A report: it warns of nothing,
gates nothing and changes no fit.
"""
from collections import namedtuple
from time import time

import numpy as np

from gpry_amd.maximize import _inv_spd

HyperLaplace = namedtuple("HyperLaplace", ["theta", "names", "lml", "grad", "H", "bounds", "free", "negdef", "cov", "sigma_log",
                                           "corr", "eigvals", "eigvecs", "log_evidence", "device_s", "wall_s"])
HyperLaplace.__doc__ = """What ``hyper_laplace`` returns, in the device's own vector theta = [log C, log l_1 .. log l_d] and
log w last for a model with a ``WhiteKernel`` (p entries, ``names``: "log C", "log l_k", "log w"), transformed units.
lml, grad (p,), H (p, p): the log marginal likelihood and its first two derivatives at theta.  bounds (p, 2): the kernel's log
bounds (a fixed hyper-parameter: its value twice).  free (p,) bool: the entries the approximation is over -- not declared
fixed, not sitting on a bound with the gradient pointing outward.  With H_ff the Hessian over the k free entries: negdef
says whether -H_ff has a Cholesky factor; cov (k, k) = (-H_ff)^-1, None when it has none; sigma_log (p,): the standard
deviation of each entry (NaN where held or not negdef); corr (k, k): the correlation matrix of cov (None with it); eigvals
(k,) ascending and eigvecs (k, k; columns) of -H_ff, so that the sloppiest direction comes first.
log_evidence = lml + (k / 2) log 2 pi - (1 / 2) log det(-H_ff) - sum_free log(hi - lo): the Laplace evidence of the kernel
family under a flat prior in log theta over the bounds (the convention of ``LaplaceResult.logZ``), NaN unless every entry
is free and negdef holds.  device_s / wall_s: time in the device call / in the whole function."""

ON_BOUND_ATOL = 1e-10       # theta goes through exp and log on its way into the kernel: "on the bound" up to that rounding


def _full_layout(kernel, d, theta_full):
    """(bounds (p, 2), fixed (p,)) of the device's vector from the kernel's own entries."""
    p = len(theta_full)
    M = np.stack([kernel.grad_from_full(e, d) for e in np.eye(p)], axis=1)      # kernel entries x device entries
    if np.any(M.sum(axis=1) > 1):
        raise ValueError("hyper_laplace: an isotropic length scale ties several entries of the device's theta; give the "
                         "kernel one length scale per dimension")
    kb = np.atleast_2d(np.asarray(kernel.bounds, dtype=float)).reshape(-1, 2)
    bounds = np.column_stack([theta_full, theta_full]).astype(float)
    fixed = np.ones(p, dtype=bool)
    for k in range(M.shape[0]):
        i = int(np.argmax(M[k]))
        bounds[i] = kb[k]
        fixed[i] = False
    return bounds, fixed


def hyper_laplace(gpr, theta=None):
    """The Gaussian approximation of the marginal likelihood in theta at ``theta`` (the kernel's own entries; None: the
    fitted ``kernel_.theta``): a ``HyperLaplace``.  One device call (``gpr.lml_hessian``'s: d products of 2 N^3 flop; models
    of more than 4096 padded rows are refused), counted as one evaluation in ``gpr.n_eval_loglike``.

    ``sigma_log`` says which length scales the data pin and which are sloppy, ``corr`` whether log C and the length
    scales are degenerate, ``free`` whether an entry sits on its bound because the optimiser was stopped there.

    ``log_evidence`` is good for comparing kernel families fitted to the SAME training set (same X, y, noise and
    preprocessing): the family with the larger value is favoured, and the difference is a log Bayes factor under flat
    priors in log theta over each kernel's bounds -- so it depends on those bounds.  It is NOT an evidence when an entry
    is held by its bound or -H_ff is not positive definite: the Gaussian integral does not describe such a maximum, and
    the field is NaN there.  Nor is it the evidence Z of the sampled posterior (``laplace_gp``, the nested sampler)."""
    t_start = time()
    kernel, th, out = gpr._lml_hessian_full(theta)
    d = gpr.d
    p = len(th)
    names = ["log C"] + [f"log l_{k + 1}" for k in range(d)] + (["log w"] if p == d + 2 else [])
    bounds, fixed = _full_layout(kernel, d, th)
    lo, hi = bounds[:, 0], bounds[:, 1]
    g, H = np.asarray(out["grad"], dtype=float), np.asarray(out["H"], dtype=float)
    at_lo = np.isclose(th, lo, rtol=0.0, atol=ON_BOUND_ATOL)
    at_hi = np.isclose(th, hi, rtol=0.0, atol=ON_BOUND_ATOL)
    free = ~fixed & ~(at_lo & (g <= 0)) & ~(at_hi & (g >= 0))
    k = int(free.sum())
    ok = np.isfinite(out["lml"])
    A = -H[np.ix_(free, free)]
    inv = (_inv_spd(A) if k else (np.zeros((0, 0)), 0.0)) if ok else None
    negdef = inv is not None
    sigma = np.full(p, np.nan)
    cov = corr = None
    if negdef:
        cov = inv[0]
        s = np.sqrt(np.diag(cov))
        sigma[free] = s
        corr = cov / np.outer(s, s)
    if ok and k:
        eigvals, eigvecs = np.linalg.eigh(A)
    else:
        eigvals, eigvecs = np.zeros(0), np.zeros((k, 0))
    log_evidence = np.nan
    if negdef and k == p:
        log_evidence = out["lml"] + 0.5 * k * np.log(2.0 * np.pi) - 0.5 * inv[1] - float(np.sum(np.log(hi - lo)))
    return HyperLaplace(theta=th, names=names, lml=float(out["lml"]), grad=g, H=H, bounds=bounds, free=free, negdef=negdef,
                        cov=cov, sigma_log=sigma, corr=corr, eigvals=eigvals, eigvecs=eigvecs, log_evidence=float(log_evidence),
                        device_s=out["device_ms"] / 1e3, wall_s=time() - t_start)
