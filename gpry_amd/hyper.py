"""How well the data determine the hyper-parameters: the Laplace approximation of the marginal likelihood in theta.

``hyper_laplace(gpr)`` evaluates the log marginal likelihood, its gradient and its Hessian at theta in one device call
(``gpry_lml_hessian``, closed form) and reads from them which entries the data pin and which are sloppy, how they are
correlated, which are held by a bound, and the Laplace evidence of the kernel family.  A report: it warns of nothing,
gates nothing and changes no fit.  ``hyper_spread`` carries the Gaussian's draws of theta to a Monte Carlo sample of the
posterior, ``hyper_predict`` to the predictive mean and error bar at given points, ``hyper_acq_spread`` -- to first order --
to sigma and the LogExp acquisition at given points and to their ranking.
"""
import warnings
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


def _theta_draws(gpr, who, n_draws, seed, laplace, scale):
    """The draws of theta that ``hyper_spread`` and ``hyper_predict`` share: the argument checks, the Laplace report
    (``laplace``; None: ``hyper_laplace(gpr)``) and ``dtheta`` (n_draws, p) ~ N(0, scale^2 cov) over the free entries from
    ``np.random.default_rng(seed)`` through the Cholesky factor of cov, zero in the held entries.  Returns
    ``(n_draws, seed, scale, lap, free, cov, dtheta)``."""
    n_draws, scale = int(n_draws), float(scale)
    if n_draws < 2:
        raise ValueError(f"n_draws must be at least 2 (got {n_draws})")
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError(f"scale must be positive and finite (got {scale})")
    if seed is None:
        seed = int(np.random.default_rng().integers(2**63 - 1))
    seed = int(seed)
    lap = hyper_laplace(gpr) if laplace is None else laplace
    if not lap.negdef or lap.cov is None:
        raise ValueError(f"{who}: negdef is False -- minus the Hessian of the log marginal likelihood over the free "
                         "entries is not positive definite, there is no covariance of theta to draw from")
    free = np.asarray(lap.free, dtype=bool)
    k = int(free.sum())
    if k == 0:
        raise ValueError(f"{who}: no entry of theta is free (all are fixed or held by a bound): nothing to draw")
    cov = np.asarray(lap.cov, dtype=float)
    dtheta = np.zeros((n_draws, len(free)))
    dtheta[:, free] = scale * np.random.default_rng(seed).standard_normal((n_draws, k)).dot(np.linalg.cholesky(cov).T)
    return n_draws, seed, scale, lap, free, cov, dtheta


def _theta_weights(lap, free, cov, dtheta, scale, lml, lml0, ok):
    """``(theta_logw, tw, theta_ess)`` of the draws: the log ratio of the marginal likelihood to the Laplace Gaussian the
    draw came from, ``lml_s - lml0 + dtheta_s^T cov^-1 dtheta_s / (2 scale^2)`` over the free entries (-inf for a draw that
    leaves ``lap.bounds`` or is not ``ok``), ``tw = exp(theta_logw - max)`` (zeros when no draw has a weight) and its Kish
    effective sample size."""
    th0 = np.asarray(lap.theta, dtype=float)
    quad = 0.5 * np.einsum("sf,fg,sg->s", dtheta[:, free], np.linalg.inv(cov), dtheta[:, free]) / scale ** 2
    bounds = np.asarray(lap.bounds, dtype=float)
    th_s = th0[None, :] + dtheta
    inside = np.all((th_s[:, free] >= bounds[free, 0]) & (th_s[:, free] <= bounds[free, 1]), axis=1)
    with np.errstate(invalid="ignore"):
        theta_logw = np.where(inside & ok, lml - lml0 + quad, -np.inf)
    tw = np.exp(theta_logw - theta_logw.max()) if np.isfinite(theta_logw.max()) else np.zeros(len(dtheta))
    return theta_logw, tw, float(tw.sum() ** 2 / np.sum(tw * tw)) if tw.any() else 0.0


class HyperSpread:
    """What ``hyper_spread`` returns.  Per draw s (arrays of length ``n_draws``): ``dtheta`` (n_draws, p; the draw in the
    device's vector, zero in the held entries), ``dlogZ`` (the change of log Z), ``means`` (n_draws, d), ``covs``
    (n_draws, d, d) and ``ess`` (Kish) of the sample reweighted under draw s.  Summaries, those of ``SurrogateSpread``:
    ``mean0`` / ``cov0`` (the sample's own mean and covariance), ``logZ_std``, ``mean_shift_sigma`` (d,; the std over draws
    of the mean in units of the baseline posterior sigma), ``cov_ratio_std`` (d,; the std over draws of var_s / var_0 per
    parameter), ``ess_min``.  ``sigma_theta`` (n_points,): sqrt(G cov G^T) per kept row, the part of the mean's error bar
    that comes from theta (times ``scale``).  ``max_abs_logr``: the largest |log r_si|, the reach of the linearisation --
    beyond about 1 the first order is only indicative.  ``keep`` (the indices of the rows that take part), ``n_points``,
    ``device_ms``, ``seed``, ``scale``.

    ``exact``: False for the first-order mode, in which the fields below are None.  With ``hyper_spread(..., exact=True)``
    log r_si is the refactorised change of the mean, ``mean_s(x_i) - mean_0(x_i)`` from one ``predict_thetas`` call, and
    everything above is computed from it by the same code, UNWEIGHTED over the draws as in the first-order mode, so that
    the two stay comparable (``theta_logw`` is reported, not applied).  ``lml`` (n_draws,) and ``lml0``: the log marginal
    likelihood at theta + dtheta_s and at theta.  ``failed`` (n_draws,) bool: the draws whose matrix was not positive
    definite; they take no part in any summary and their per-draw entries are NaN.  ``sigma_theta_draws`` (n_points,):
    the std over the surviving draws of ``mean_s(x_i)``, the non-linear twin of ``sigma_theta`` (which stays the
    linearised one).  ``first_order_miss``: the largest ``|log r_exact - G . dtheta|`` over the rows that take part and
    the surviving draws -- how wrong the first-order mode would have been.  ``theta_logw`` (n_draws,):
    ``lml_s - lml0 + dtheta_s^T cov^-1 dtheta_s / (2 scale^2)`` over the free entries, the log ratio of the marginal
    likelihood to the Laplace Gaussian the draw came from (about 0 where Laplace is good; -inf for a draw that leaves the
    kernel's bounds, ``HyperLaplace.bounds``, or failed).  ``theta_ess``: the Kish effective sample size of
    ``exp(theta_logw)``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"HyperSpread(n_points={self.n_points}, n_draws={len(self.dlogZ)}, logZ_std={self.logZ_std:.3g}, "
                f"mean_shift_sigma={np.array2string(np.asarray(self.mean_shift_sigma), precision=3)}, "
                f"ess_min={self.ess_min:.1f}, max_abs_logr={self.max_abs_logr:.3g})")


def reweight(wk, Xk, logr):
    """The sample ``Xk`` (m, d) with normalised weights ``wk`` reweighted by each row of ``logr`` (S, m; -inf: the row
    takes no part): ``(dlogZ, ws, ess, means, covs, mean0, cov0)`` -- log sum_i w_i r_si, the normalised weights w_i r_si,
    their Kish effective sample size, mean and covariance under them, and the sample's own mean and covariance.  What
    ``hyper_spread`` and ``mc.batch_influence`` make their reports of."""
    d = Xk.shape[1]
    top = logr.max(axis=1)
    e = wk[None, :] * np.exp(logr - top[:, None])
    tot = e.sum(axis=1)
    dlogZ = top + np.log(tot)
    ws = e / tot[:, None]
    ess = 1.0 / np.sum(ws * ws, axis=1)
    means = ws.dot(Xk)
    covs = np.empty((len(logr), d, d))
    for s in range(len(logr)):                          # weighted Grams, one draw at a time: O(M d) beside ws
        cen = Xk - means[s]
        covs[s] = (cen * ws[s][:, None]).T.dot(cen)
    mean0 = wk.dot(Xk)
    cen0 = Xk - mean0
    cov0 = (cen0 * wk[:, None]).T.dot(cen0)
    return dlogZ, ws, ess, means, covs, mean0, cov0


def hyper_spread(gpr, X, y, w=None, n_draws=256, seed=None, laplace=None, scale=1.0, exact=False):
    """How far the posterior moves because theta is only known as well as the data pin it: the Monte Carlo sample
    ``(X, y, w)`` that ``mc_sample_from_gp`` returned, reweighted to first order under ``n_draws`` draws
    dtheta_s ~ N(0, scale^2 cov) of the hyper-parameters, cov the Laplace covariance of ``hyper_laplace`` (``laplace``: a
    ``HyperLaplace``; None: ``hyper_laplace(gpr)``).  The twin of ``surrogate_spread``, which takes theta as given.

    With G = d mean / d theta at the rows (``gpr.mean_theta_grad(X, full=True)``, one device call, any number of rows):
    log r_si = G(x_i) . dtheta_s, dlogZ_s = log sum_i w_i r_si, and mean, covariance and Kish effective sample size of the
    weights w_i r_si.  The rows are those of positive finite weight and finite y; rows the gates reject take no part.
    Entries of theta that are not ``free`` are held: their draws are zero.  The draws come from
    ``np.random.default_rng(seed)`` through the Cholesky factor of cov (None: fresh entropy).

    Raises a ValueError when ``laplace.negdef`` is false (there is no covariance to draw from) or no entry is free.
    Warns when the smallest effective sample size is below 5 % of the rows.  Host memory is O(n_draws M + M d^2).
    Returns a ``HyperSpread``.

    ``exact=True``: the same draws from the same seed, but log r_si = mean_s(x_i) - mean_0(x_i) with the model
    REFACTORISED at theta + dtheta_s -- one ``gpr.predict_thetas`` call (``gpry_predict_thetas``) with theta itself as its
    first row, so that a draw that does not move theta has log r = 0 exactly; theta is ``laplace.theta``.  The fitted model
    is not touched.  Everything downstream of log r is the code of the first-order mode, and the summaries stay UNWEIGHTED
    over the draws, so that the two modes remain comparable: ``theta_logw`` says how far the Laplace Gaussian is from the
    marginal likelihood at each draw and is not applied.  The first-order call is still made (it decides which rows the
    gates reject, and ``first_order_miss`` compares the two).  A draw whose matrix is not positive definite is dropped
    from every summary and flagged in ``failed``; a ValueError is raised when all fail.  See ``HyperSpread`` for the
    fields this mode adds."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    y = np.asarray(y, dtype=float)
    n, d = X.shape
    w = np.full(n, 1.0 / max(n, 1)) if w is None else np.asarray(w, dtype=float)
    if y.shape != (n,) or w.shape != (n,):
        raise ValueError(f"expected y and w of shape ({n},), got {y.shape} and {w.shape}")
    n_draws, seed, scale, lap, free, cov, dtheta = _theta_draws(gpr, "hyper_spread", n_draws, seed, laplace, scale)
    keep = np.flatnonzero((w > 0) & np.isfinite(w) & np.isfinite(y))
    if len(keep) == 0:
        raise ValueError("the sample has no row of positive weight and finite y")
    wk = w[keep] / w[keep].sum()
    Xk = np.ascontiguousarray(X[keep])
    m = len(keep)
    res = gpr._mean_theta_grad_full(Xk)
    G = np.asarray(res["G"], dtype=float)
    p = len(free)
    if G.shape != (m, p):
        raise ValueError(f"hyper_spread: the Laplace report has {p} entries of theta, the model {G.shape[1]}")
    Gf = G[:, free]
    sigma_theta = np.sqrt(np.maximum(np.einsum("if,fg,ig->i", Gf, cov, Gf), 0.0)) * scale
    logr = dtheta.dot(G.T)                              # (n_draws, m)
    alive = np.isfinite(res["y"])                       # rows the gates reject take no part
    if not alive.any():
        raise ValueError("every row of the sample is rejected by the classifier or the trust region")
    device_ms = res["device_ms"]
    more = dict(exact=False, lml=None, lml0=None, failed=None, sigma_theta_draws=None, first_order_miss=None, theta_logw=None,
                theta_ess=None)
    ok = None                                           # exact mode: the draws that take part
    if exact:
        th0 = np.asarray(lap.theta, dtype=float)
        pt = gpr._predict_thetas_full(Xk, np.vstack([th0[None, :], th0[None, :] + dtheta]))
        if pt["info"][0] != 0:
            raise ValueError("hyper_spread: the matrix at theta itself is not positive definite")
        failed = np.asarray(pt["info"][1:]) != 0
        if failed.all():
            raise ValueError(f"hyper_spread: the matrix is not positive definite at any of the {n_draws} draws of theta")
        ok = ~failed
        mean_s = pt["mean"][1:][ok]
        linear = logr[ok]
        logr = mean_s - pt["mean"][0][None, :]
        lml0, lml = float(pt["lml"][0]), np.asarray(pt["lml"][1:], dtype=float)
        theta_logw, _, theta_ess = _theta_weights(lap, free, cov, dtheta, scale, lml, lml0, ok)
        more = dict(exact=True, lml=lml, lml0=lml0, failed=failed, sigma_theta_draws=mean_s.std(axis=0),
                    first_order_miss=float(np.max(np.abs(logr[:, alive] - linear[:, alive]))), theta_logw=theta_logw,
                    theta_ess=theta_ess)
        device_ms = device_ms + pt["device_ms"]
        del pt, mean_s, linear
    max_abs_logr = float(np.max(np.abs(logr[:, alive])))
    logr[:, ~alive] = -np.inf
    dlogZ, ws, ess, means, covs, mean0, cov0 = reweight(wk, Xk, logr)
    var0 = np.diag(cov0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_shift_sigma = means.std(axis=0) / np.sqrt(var0)
        cov_ratio_std = (np.einsum("saa->sa", covs) / var0).std(axis=0)
    logZ_std, ess_min = float(dlogZ.std()), float(ess.min())
    if ok is not None and not ok.all():                 # the per-draw arrays keep their length: NaN where the draw failed
        def spread(a):
            full = np.full((n_draws,) + a.shape[1:], np.nan)
            full[ok] = a
            return full
        dlogZ, means, covs, ess = spread(dlogZ), spread(means), spread(covs), spread(ess)
    out = HyperSpread(dtheta=dtheta, dlogZ=dlogZ, means=means, covs=covs, ess=ess, mean0=mean0, cov0=cov0,
                      logZ_std=logZ_std, mean_shift_sigma=mean_shift_sigma, cov_ratio_std=cov_ratio_std,
                      ess_min=ess_min, sigma_theta=sigma_theta, max_abs_logr=max_abs_logr, keep=keep, n_points=m,
                      device_ms=device_ms, seed=seed, scale=scale, **more)
    if out.ess_min < 0.05 * m:
        warnings.warn(f"hyper_spread: the smallest effective sample size over the draws is {out.ess_min:.1f} of {m} "
                      "rows (< 5 %): the hyper-parameters are too uncertain for the reweighted sample to mean anything")
    return out


class HyperPredict:
    """What ``hyper_predict`` returns, at the M rows of X in untransformed units.  ``mean0``, ``sigma0`` (M,): mean and
    sigma at the fitted theta (row 0 of the call: the unclipped mean and ``sqrt(max(var, 0))``).  Over the surviving draws
    of theta: ``mean`` (the average of the draws' means), ``sigma_gp`` (the square root of the average of
    ``max(var_s, 0)``: the GP's own error bar, averaged over theta), ``sigma_theta`` (the standard deviation of the draws'
    means: what theta's uncertainty adds), ``sigma_total = sqrt(sigma_gp^2 + sigma_theta^2)`` (the law of total variance)
    and ``inflation = sigma_total / sigma0`` (inf or NaN where sigma0 is 0).  Per draw s (length ``n_draws``, NaN where
    the draw failed): ``dtheta`` (n_draws, p), ``means`` and ``vars`` (n_draws, M; the variance as the device returns it,
    not clamped), ``lml``.  ``lml0``; ``failed`` (n_draws,) bool: the draws whose matrix was not positive definite, left
    out of every summary; ``theta_logw`` (n_draws,) and ``theta_ess``: as in ``HyperSpread``.  ``weighted``: whether the
    summaries use the self-normalised weights ``exp(theta_logw)``.  ``device_ms``, ``seed``, ``scale``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"HyperPredict(n_points={len(self.mean0)}, n_draws={len(self.lml)}, failed={int(np.sum(self.failed))}, "
                f"max inflation={np.nanmax(self.inflation):.3g}, theta_ess={self.theta_ess:.1f}, weighted={self.weighted})")


def hyper_predict(gpr, X, n_draws=64, seed=None, laplace=None, scale=1.0, weighted=False):
    """The predictive at the rows of ``X`` (M, d) with the hyper-parameters marginalised over the Laplace Gaussian of
    ``hyper_laplace``: by the law of total variance the error bar at x is
    ``E_theta[sigma^2(x | theta)] + Var_theta[mean(x | theta)]``.  The draws are ``hyper_spread``'s -- the same Gaussian
    (``laplace``: a ``HyperLaplace``; None: ``hyper_laplace(gpr)``), the same seed convention, entries that are not free
    held -- with the fitted theta (``laplace.theta``) in front as row 0 of ONE ``gpr.predict_thetas`` call
    (``gpry_predict_thetas_var``: one refactorisation per draw, mean and variance of every draw at every point).  The
    fitted model is not touched.  Returns a ``HyperPredict``.

    The summaries are UNWEIGHTED over the draws by default, comparable with ``hyper_spread``; ``weighted=True`` applies
    the self-normalised importance weights ``exp(theta_logw)`` (the marginal likelihood over the Laplace Gaussian, zero
    for a draw outside the kernel's bounds), computed as in ``hyper_spread(exact=True)``.  A report: it changes no
    default anywhere.  Raises a ValueError when there is no covariance to draw from, when the matrix at theta itself or
    at every draw is not positive definite, or when ``weighted`` leaves no draw with a weight."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    n_draws, seed, scale, lap, free, cov, dtheta = _theta_draws(gpr, "hyper_predict", n_draws, seed, laplace, scale)
    th0 = np.asarray(lap.theta, dtype=float)
    pt = gpr._predict_thetas_full(X, np.vstack([th0[None, :], th0[None, :] + dtheta]), want_var=True)
    if pt["info"][0] != 0:
        raise ValueError("hyper_predict: the matrix at theta itself is not positive definite")
    failed = np.asarray(pt["info"][1:]) != 0
    if failed.all():
        raise ValueError(f"hyper_predict: the matrix is not positive definite at any of the {n_draws} draws of theta")
    ok = ~failed
    means, vars_ = np.array(pt["mean"][1:], dtype=float), np.array(pt["var"][1:], dtype=float)
    means[failed], vars_[failed] = np.nan, np.nan
    lml0, lml = float(pt["lml"][0]), np.asarray(pt["lml"][1:], dtype=float)
    theta_logw, tw, theta_ess = _theta_weights(lap, free, cov, dtheta, scale, lml, lml0, ok)
    if weighted:
        if not tw.any():
            raise ValueError("hyper_predict: weighted=True and no draw of theta has a weight (all failed or left the bounds)")
        wts = tw[ok] / tw[ok].sum()
    else:
        wts = np.full(int(ok.sum()), 1.0 / int(ok.sum()))
    m_ok, v_ok = means[ok], np.maximum(vars_[ok], 0.0)
    mean = wts.dot(m_ok)
    sigma_gp = np.sqrt(wts.dot(v_ok))
    sigma_theta = np.sqrt(wts.dot((m_ok - mean[None, :]) ** 2))
    sigma_total = np.sqrt(sigma_gp ** 2 + sigma_theta ** 2)
    mean0 = np.array(pt["mean"][0], dtype=float)
    sigma0 = np.sqrt(np.maximum(pt["var"][0], 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        inflation = sigma_total / sigma0
    return HyperPredict(mean0=mean0, sigma0=sigma0, mean=mean, sigma_gp=sigma_gp, sigma_theta=sigma_theta,
                        sigma_total=sigma_total, inflation=inflation, dtheta=dtheta, means=means, vars=vars_, lml=lml, lml0=lml0,
                        failed=failed, theta_logw=theta_logw, theta_ess=theta_ess,
                        weighted=bool(weighted), device_ms=pt["device_ms"], seed=seed, scale=scale)


class HyperAcqSpread:
    """What ``hyper_acq_spread`` returns, at the n rows of X in untransformed units, theta in the device's own vector
    (p entries).  ``mean`` (``predict`` of the row: clip and gates included, -inf for a gated row), ``var`` (the latent
    variance, not clamped) and ``sigma = sqrt(max(var, 0))``; ``G_mean``, ``G_var`` (n, p): their derivatives in theta.
    ``sigma_mean_theta`` = sqrt(g_m^T S g_m) with S = scale^2 cov over the free entries (``hyper_spread``'s
    ``sigma_theta``), ``sigma_rel_theta`` = sqrt(g_v^T S g_v) / (2 var): the relative standard deviation of sigma itself
    (NaN where var <= 0).  ``acq`` (n,): LogExp's value 2 zeta (mean - y_max) + log(var - sigma_n^2) / 2, -inf for a dead row
    (var <= sigma_n^2 or a mean that is not finite); ``acq_grad`` (n, p) = 2 zeta G_mean + G_var / (2 (var - sigma_n^2)), NaN
    for a dead row; ``acq_sigma_theta`` (n,) = sqrt(g_a^T S g_a), NaN for a dead row.  ``order`` (n,): the rows by
    descending ``acq`` (dead rows last, ties in input order).  ``flip`` (n, n; None above 256 rows):
    Phi(-|a_i - a_j| / s_ij) with s_ij^2 = (g_i - g_j)^T S (g_i - g_j), the first-order probability that rows i and j swap rank
    under a draw of theta; 1/2 on the diagonal, 0 where s_ij = 0 and the values differ, NaN where either row is dead.
    ``top_flip`` (n,): the same against the top row ``order[0]`` -- 0 for that row itself, NaN for dead rows.  ``zeta``,
    ``sigma_n``, ``baseline`` (``gpr.y_max``), ``free``, ``scale``, ``device_ms`` (the two device calls)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        live = np.isfinite(self.acq)
        top = np.nanmax(self.top_flip) if live.any() else np.nan
        return (f"HyperAcqSpread(n_points={len(self.acq)}, live={int(live.sum())}, zeta={self.zeta:.3g}, "
                f"max top_flip={top:.3g})")


FLIP_MAX_ROWS = 256         # the (n, n) table of pairwise swap probabilities is given up to this many rows


def _phi_neg(z):
    """Phi(-z), the standard normal's lower tail, elementwise (NaN stays NaN)."""
    from math import erfc
    return 0.5 * np.vectorize(erfc, otypes=[float])(np.asarray(z, dtype=float) / np.sqrt(2.0))


def _swap_probability(a_i, a_j, s):
    """Phi(-|a_i - a_j| / s) with the limits at s = 0: 1/2 where the values are equal too, 0 where they differ."""
    gap = np.abs(a_i - a_j)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(s > 0.0, gap / s, np.where(gap > 0.0, np.inf, 0.0))
    return _phi_neg(np.where(np.isnan(gap) | np.isnan(s), np.nan, z))


def acq_spread_fields(mean, var, G_mean, G_var, cov_free, free, zeta, sigma_n, baseline, scale=1.0):
    """The fields of ``HyperAcqSpread`` that are arithmetic on the two device results: a dict.  ``cov_free`` (k, k): the
    covariance of theta over the ``free`` entries (p,) bool.  Kept apart from the device calls so that it can be checked
    on the host alone."""
    mean, var = np.asarray(mean, dtype=float), np.asarray(var, dtype=float)
    G_mean, G_var = np.asarray(G_mean, dtype=float), np.asarray(G_var, dtype=float)
    free = np.asarray(free, dtype=bool)
    S = float(scale) ** 2 * np.asarray(cov_free, dtype=float)
    n = len(mean)

    def spread(G):
        Gf = G[:, free]
        return np.sqrt(np.maximum(np.einsum("if,fg,ig->i", Gf, S, Gf), 0.0))

    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = np.sqrt(np.maximum(var, 0.0))
        sigma_rel_theta = np.where(var > 0.0, spread(G_var) / (2.0 * var), np.nan)
        excess = var - sigma_n ** 2
        live = (excess > 0.0) & np.isfinite(mean)
        acq = np.where(live, 2.0 * zeta * (mean - baseline) + 0.5 * np.log(np.where(live, excess, 1.0)), -np.inf)
        acq_grad = np.full(G_var.shape, np.nan)
        acq_grad[live] = 2.0 * zeta * G_mean[live] + G_var[live] / (2.0 * excess[live])[:, None]
    acq_sigma_theta = np.full(n, np.nan)
    acq_sigma_theta[live] = spread(acq_grad[live])
    order = np.argsort(-acq, kind="stable")
    a_nan = np.where(live, acq, np.nan)
    Af = acq_grad[:, free]

    def pair_sd(Di):                                    # sqrt(D S D^T) row by row
        return np.sqrt(np.maximum(np.einsum("...f,fg,...g->...", Di, S, Di), 0.0))

    flip = None
    if n <= FLIP_MAX_ROWS:
        flip = _swap_probability(a_nan[:, None], a_nan[None, :], pair_sd(Af[:, None, :] - Af[None, :, :]))
    top_flip = np.full(n, np.nan)
    if live.any():
        top = int(order[0])
        top_flip = _swap_probability(a_nan, a_nan[top], pair_sd(Af - Af[top][None, :]))
        top_flip[top] = 0.0
    return dict(sigma=sigma, sigma_mean_theta=spread(G_mean), sigma_rel_theta=sigma_rel_theta, acq=acq, acq_grad=acq_grad,
                acq_sigma_theta=acq_sigma_theta, order=order, flip=flip, top_flip=top_flip)


def hyper_acq_spread(gpr, X, acq=None, laplace=None, scale=1.0):
    """Would another plausible theta have ranked these proposals differently?  At the rows of ``X`` (n, d) -- a NORA
    shortlist, the last proposals -- the spread of sigma and of the LogExp acquisition
    2 zeta (mean - y_max) + log(sigma^2 - sigma_n^2) / 2 under the Laplace Gaussian of ``hyper_laplace`` (``laplace``: a
    ``HyperLaplace``; None: ``hyper_laplace(gpr)``; ``scale`` multiplies its standard deviations), and the probability
    that two rows swap rank.  Two device calls, ``gpr.mean_theta_grad(full=True)`` and ``gpr.var_theta_grad(full=True)``
    (closed forms, no refactorisation; models of more than 4096 padded rows are refused by the latter).  zeta and sigma_n
    come from ``acq``, a ``gpry_amd.acquisition_functions.LogExp`` (None: ``LogExp(dimension=d)``), sigma_n resolved as
    ``LogExp`` resolves it for the value (its own, else the mean of ``gpr.noise_level``); the baseline is ``gpr.y_max``.
    A row whose variance does not exceed sigma_n^2 or whose mean is not finite (a gated row) is dead, as for the
    acquisition itself: ``acq`` -inf, its derivative NaN.

    FIRST ORDER ONLY: every figure is the linearisation of mean and variance in theta at the fitted theta, carried through
    a Gaussian -- good while ``acq_sigma_theta`` is well below 1 and theta's Gaussian is narrow.  The exact route is
    ``gpr.predict_thetas(X, thetas, return_std=True)`` over draws of theta (``hyper_predict``'s call), one
    refactorisation per draw.  A report: it warns of nothing, gates nothing and changes no default.

    Raises the ValueErrors of ``hyper_spread`` when ``laplace.negdef`` is false (there is no covariance) or no entry of
    theta is free.  Returns a ``HyperAcqSpread``."""
    from gpry_amd.acquisition_functions import LogExp
    X = np.atleast_2d(np.asarray(X, dtype=float))
    scale = float(scale)
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError(f"scale must be positive and finite (got {scale})")
    lap = hyper_laplace(gpr) if laplace is None else laplace
    if not lap.negdef or lap.cov is None:
        raise ValueError("hyper_acq_spread: negdef is False -- minus the Hessian of the log marginal likelihood over the free "
                         "entries is not positive definite, there is no covariance of theta to draw from")
    free = np.asarray(lap.free, dtype=bool)
    if int(free.sum()) == 0:
        raise ValueError("hyper_acq_spread: no entry of theta is free (all are fixed or held by a bound): nothing to draw")
    acq = LogExp(dimension=X.shape[1]) if acq is None else acq
    zeta, sigma_n = float(acq.zeta), float(acq._noise(gpr)[0])
    rm = gpr._mean_theta_grad_full(X)
    rv = gpr._var_theta_grad_full(X)
    G_mean, G_var = np.asarray(rm["G"], dtype=float), np.asarray(rv["G"], dtype=float)
    if G_var.shape != (len(X), len(free)):
        raise ValueError(f"hyper_acq_spread: the Laplace report has {len(free)} entries of theta, the model {G_var.shape[1]}")
    mean, var = np.asarray(rm["y"], dtype=float), np.asarray(rv["var"], dtype=float)
    baseline = float(gpr.y_max)
    fields = acq_spread_fields(mean, var, G_mean, G_var, lap.cov, free, zeta, sigma_n, baseline, scale)
    return HyperAcqSpread(mean=mean, var=var, G_mean=G_mean, G_var=G_var, zeta=zeta, sigma_n=sigma_n, baseline=baseline,
                          free=free, scale=scale, device_ms=rm["device_ms"] + rv["device_ms"], **fields)
