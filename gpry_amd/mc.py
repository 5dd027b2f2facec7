"""The Monte Carlo sample of the surrogate that a run ends with (gpry/mc.py), made on the device.

``mc_sample_from_gp(gpr, sampler="nested" | "mcmc" | "hmc" | "tempered")`` runs one of the device samplers of the
surrogate's mean: the nested sampler of ``gpry_amd/nested.py`` in place of PolyChord / UltraNest (gpry/mc.py:328-456), or,
in place of Cobaya's MCMC (gpry/mc.py:173-327), the Metropolis chains of ``gpry_amd/mcmc.py``, the Hamiltonian chains of
``gpry_amd/hmc.py`` or the tempered Metropolis ladders of ``gpry_amd/tempering.py``.  All evaluate
``gpr.predict(x[None])`` bit for bit, the classifier and trust region included.
``mc_sample_from_gp_ns`` keeps the reference's signature, so that ``gpry_amd.integration.patch_gpry_mc`` can put it
under an unmodified ``Runner.generate_mc_sample``.
"""
import os
import warnings

import numpy as np

from gpry_amd.maximize import (hessian_gp, laplace_covmat, laplace_gp, maximize_acq, maximize_gp,  # noqa: F401
                               profile_gp)  # (beside mc_sample_from_gp: the best fit, its curvature and profiles)
from gpry_amd.hyper import HyperLaplace, hyper_laplace  # noqa: F401  (... and the curvature of the marginal likelihood in theta)
from gpry_amd.hyper import HyperSpread, hyper_spread  # noqa: F401  (... and what it does to the posterior: to first order, or with exact=True refactorised per draw)
from gpry_amd.hyper import reweight as _reweight
from gpry_amd.hyper import HyperAcqSpread, hyper_acq_spread  # noqa: F401  (... and to sigma and the LogExp acquisition at given points: would another plausible theta rank them differently)
from gpry_amd.hyper import HyperPredict, hyper_predict  # noqa: F401  (... and to the error bar at a point: mean and sigma with theta marginalised)
from gpry_amd.tools import generic_params_names, get_Xnumber

# PolyChord's defaults (the Runner passes nlive = 50d)
NESTED_DEFAULTS = {"nlive": "25d", "num_repeats": "5d", "precision_criterion": 0.001, "nprior": None, "max_ncalls": None}
# options of the device nested sampler beyond PolyChord's settings: in nested_settings' result only when given
NESTED_EXTRA = {"clustering": False, "cluster_volumes": False, "phantom_thin": None}
# PolyChord's names of those options -> ours, for the warning that ignores them
NESTED_RENAMED = {"do_clustering": "clustering"}
# Cobaya's names where they exist -> run_mcmc's arguments
MCMC_KEYS = {"Rminus1_stop": "Rminus1_stop", "temperature": "temperature", "covmat": "covmat",
             "max_samples": "max_ncalls", "max_ncalls": "max_ncalls", "nchains": "nchains", "learn_every": "learn_every",
             "learn_batches": "learn_batches", "batch_steps": "batch_steps", "max_batches": "max_batches",
             "thin": "thin", "skip": "skip", "reset_temperature": "reset_temperature"}


def _known(options, keys, sampler, renamed=None):
    """The entries of ``options`` whose key is in ``keys``; a warning for the rest (gpry/ns_interfaces.py:160-170)."""
    options = dict(options or {})
    unknown = [k for k in options if k not in keys]
    if unknown:
        hint = "".join(f" Use '{renamed[k]}' for '{k}'." for k in unknown if renamed and k in renamed)
        warnings.warn(f"Options {unknown} not recognised by the device sampler '{sampler}'; they are ignored. "
                      f"Known: {sorted(keys)}.{hint}")
    return {k: v for k, v in options.items() if k in keys}


def nested_settings(d, sampler_options=None):
    """run_nested's settings from PolyChord-style options; Xnumber strings such as ``"50d"`` are multiples of d."""
    opts = dict(NESTED_DEFAULTS)
    opts.update(_known(sampler_options, {**NESTED_DEFAULTS, **NESTED_EXTRA}, "nested", NESTED_RENAMED))
    out = {}
    for k in ("nlive", "num_repeats"):
        out[k] = get_Xnumber(opts[k], "d", d, int, k)
    out["precision_criterion"] = float(opts["precision_criterion"])
    out["nprior"] = out["nlive"] if opts["nprior"] is None else get_Xnumber(opts["nprior"], "d", d, int, "nprior")
    out["max_ncalls"] = None if opts["max_ncalls"] is None else get_Xnumber(opts["max_ncalls"], "d", d, int, "max_ncalls")
    if "clustering" in opts:
        out["clustering"] = bool(opts["clustering"])
    if "cluster_volumes" in opts:
        out["cluster_volumes"] = bool(opts["cluster_volumes"])
        if out["cluster_volumes"] and not out.get("clustering"):
            raise ValueError("sampler option cluster_volumes=True needs clustering=True")
    if opts.get("phantom_thin") is not None:
        t = opts["phantom_thin"]
        if isinstance(t, bool) or int(t) != t or int(t) < 1:
            raise ValueError(f"sampler option phantom_thin = {t!r} must be an int >= 1")
        if out.get("cluster_volumes"):
            raise ValueError("sampler option phantom_thin is not available with cluster_volumes=True")
        out["phantom_thin"] = int(t)
    return out


# run_hmc's arguments: those of run_mcmc (counted in trajectories) and its own four
HMC_KEYS = {**MCMC_KEYS, "eps": "eps", "accept_target": "accept_target", "reflect": "reflect", "max_reflect": "max_reflect"}


# run_tempered's arguments: those of run_mcmc (nchains counts the ladders) and the ladder's four
TEMPERED_KEYS = {**MCMC_KEYS, "nchains": "nladders", "rungs": "rungs", "T_max": "T_max", "temperatures": "temperatures",
                 "swap_every": "swap_every"}


def _chain_settings(d, sampler_options, keys, sampler):
    """Keyword arguments of a chain sampler's run loop from Cobaya-style options; Xnumber strings such as ``"50d"``
    are multiples of d.  Unknown keys: a warning, and they are dropped (``_known``)."""
    out = {}
    for k, v in _known(sampler_options, keys, sampler).items():
        if k in ("max_samples", "max_ncalls", "nchains", "learn_every", "batch_steps", "thin", "rungs",
                 "swap_every") and v is not None:
            v = get_Xnumber(v, "d", d, int, k)
        out[keys[k]] = v
    return out


def mcmc_settings(d, sampler_options=None):
    """run_mcmc's keyword arguments from Cobaya-style options (``Rminus1_cl_stop`` and other unknown keys: a warning)."""
    return _chain_settings(d, sampler_options, MCMC_KEYS, "mcmc")


def hmc_settings(d, sampler_options=None):
    """run_hmc's keyword arguments from Cobaya-style options (unknown keys: a warning, and they are dropped)."""
    return _chain_settings(d, sampler_options, HMC_KEYS, "hmc")


def tempered_settings(d, sampler_options=None):
    """run_tempered's keyword arguments from Cobaya-style options (unknown keys: a warning, and they are dropped)."""
    return _chain_settings(d, sampler_options, TEMPERED_KEYS, "tempered")


def _string_covmat(gpr, b, s):
    """``covmat="laplace"`` among a chain sampler's settings: the covariance of the Gaussian approximation at the maximum
    of the mean in its place (``maximize.laplace_covmat``; None where that has none).  Other strings are refused."""
    if isinstance(s.get("covmat"), str):
        s["covmat"] = laplace_covmat(gpr, b, s["covmat"])


def _bounds(gpr, bounds):
    if bounds is None:
        bounds = gpr.trust_bounds if getattr(gpr, "trust_bounds", None) is not None else gpr.bounds
    return np.asarray(bounds, dtype=float)


def _push_model(gpr, sampler):
    """The model, its affine maps and the gates on the device, as NORA._do_MC_sample_nested pushes them."""
    gpr._ensure_factor()
    gpr._push_affine()
    if not gpr._push_gates():
        raise ValueError(f"sampler='{sampler}' evaluates the classifier on the device, and this classifier has no device "
                         "form")


def write_sample(output, X, y, w, params=None):
    """The reference's file (gpry/mc.py:427-455): header ``w minuslogp x_1 ...``, columns [w, -y, X]; ``.txt`` is
    appended to a name without extension and ``mc_samples.txt`` used for a bare directory.  Returns the path."""
    base_dir, file_name = os.path.split(output)
    base_dir = os.path.abspath(base_dir or os.path.curdir)
    os.makedirs(base_dir, exist_ok=True)
    root, ext = os.path.splitext(file_name or "mc_samples.txt")
    path = os.path.join(base_dir, root + (ext or ".txt"))
    if params is None:
        params = generic_params_names(X.shape[1])
    w_write = w if w is not None else np.ones(len(y))
    np.savetxt(path, np.concatenate([np.atleast_2d(w_write), np.atleast_2d(-np.asarray(y)), np.asarray(X).T]).T,
               header="w minuslogp " + " ".join(params))
    return path


def mc_sample_from_gp(gpr, bounds=None, sampler="nested", sampler_options=None, output=None, seed=None, params=None):
    """Monte Carlo sample of the surrogate's posterior mean, on the device: ``(X, y, w)``, w normalised.

    bounds: default ``gpr.trust_bounds``, else ``gpr.bounds`` (gpry/mc.py:381-382).  sampler: ``"nested"`` (options
    nlive, num_repeats, precision_criterion, nprior, max_ncalls; PolyChord's defaults 25d, 5d, 0.001, nlive; and
    clustering, default False: a whitening matrix per cluster of the live set; phantom_thin, default None: an int t
    keeps every t-th interior state of the chains as a weighted phantom row, see ``run_nested``) or
    ``"mcmc"`` (options Rminus1_stop, temperature, covmat (a matrix, or ``"laplace"``: the inverse of minus the Hessian
    of the mean at its maximum, ``laplace_gp``, for all three chain samplers), max_samples -> max_ncalls, and run_mcmc's nchains,
    learn_every, learn_batches, batch_steps, max_batches, thin, skip, reset_temperature) or ``"hmc"`` (run_hmc's
    arguments: those of "mcmc", counted in trajectories, and eps, accept_target, and reflect, default False: with
    ``{"reflect": True}`` the trajectories reflect at the walls of the box instead of being rejected there, at most
    max_reflect, default 64, times per drift) or ``"tempered"`` (run_tempered's arguments: those of "mcmc", with nchains
    the number of ladders, and rungs, default 6, T_max, temperatures, swap_every, default 5: ladders of Metropolis
    chains at rising temperatures that exchange states, for surrogates with separated modes).  Unknown options are
    warned about and ignored.  seed: int, or None for fresh entropy.  output: also write the reference's file format.
    The run's details are kept in ``mc_sample_from_gp.last_result``."""
    if not isinstance(sampler, str) or sampler.lower() not in ("nested", "mcmc", "hmc", "tempered"):
        raise ValueError(f"sampler must be 'nested', 'mcmc', 'hmc' or 'tempered', got {sampler!r}")
    sampler = sampler.lower()
    b = _bounds(gpr, bounds)
    d = len(b)
    if seed is None:
        seed = int(np.random.default_rng().integers(2**31 - 1))
    seed = int(seed)
    if sampler == "nested":
        from gpry_amd.nested import run_nested
        s = nested_settings(d, sampler_options)
        _push_model(gpr, sampler)
        res = run_nested(gpr.device, b, seed, s["nlive"], s["num_repeats"], precision_criterion=s["precision_criterion"],
                         nprior=s["nprior"], max_ncalls=s["max_ncalls"], minus_inf_value=gpr.minus_inf_value,
                         **({"clustering": True} if s.get("clustering") else {}),
                         **({"cluster_volumes": True} if s.get("cluster_volumes") else {}),
                         **({"phantom_thin": s["phantom_thin"]} if s.get("phantom_thin") else {}))
    elif sampler == "hmc":
        from gpry_amd.hmc import DEFAULT_NCHAINS, run_hmc
        s = hmc_settings(d, sampler_options)
        _string_covmat(gpr, b, s)
        nchains = s.pop("nchains", DEFAULT_NCHAINS)
        _push_model(gpr, sampler)
        res = run_hmc(gpr.device, b, seed, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value, **s)
        gpr.n_eval += res.ngrad
    elif sampler == "tempered":
        from gpry_amd.tempering import DEFAULT_NLADDERS, run_tempered
        s = tempered_settings(d, sampler_options)
        _string_covmat(gpr, b, s)
        nladders = s.pop("nladders", DEFAULT_NLADDERS)
        _push_model(gpr, sampler)
        res = run_tempered(gpr.device, b, seed, nladders, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value,
                           **s)
    else:
        from gpry_amd.mcmc import DEFAULT_NCHAINS, run_mcmc
        s = mcmc_settings(d, sampler_options)
        _string_covmat(gpr, b, s)
        nchains = s.pop("nchains", DEFAULT_NCHAINS)
        _push_model(gpr, sampler)
        res = run_mcmc(gpr.device, b, seed, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value, **s)
    gpr.n_eval += res.ncalls
    mc_sample_from_gp.last_result = res
    if output is not None:
        write_sample(output, res.X, res.y, res.w, params)
    return res.X, res.y, res.w


mc_sample_from_gp.last_result = None


class SurrogateSpread:
    """What ``surrogate_spread`` returns.  Per draw s (arrays of length ``n_draws``): ``dlogZ`` (the change of log Z),
    ``means`` (n_draws, d), ``covs`` (n_draws, d, d) and ``ess`` (Kish) of the sample reweighted under realisation s.
    Summaries: ``mean0`` / ``cov0`` (the sample's own mean and covariance), ``logZ_std``, ``mean_shift_sigma`` (d,; the
    std over draws of the mean in units of the baseline posterior sigma), ``cov_ratio_std`` (d,; the std over draws of
    var_s / var_0 per parameter), ``ess_min``, ``jitter_used``, ``n_points``, ``device_ms``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"SurrogateSpread(n_points={self.n_points}, n_draws={len(self.dlogZ)}, logZ_std={self.logZ_std:.3g}, "
                f"mean_shift_sigma={np.array2string(np.asarray(self.mean_shift_sigma), precision=3)}, "
                f"ess_min={self.ess_min:.1f})")


def _systematic(w, k, rng):
    """Systematic resampling: k indices into the normalised weights ``w`` (one uniform, k evenly spaced positions)."""
    c = np.cumsum(w)
    c[-1] = 1.0
    return np.searchsorted(c, (rng.random() + np.arange(k)) / k, side="right")


def surrogate_spread(gpr, X, y, w=None, n_draws=256, seed=None, max_points=4096, jitter=None):
    """How far the posterior moves because the GP is only an emulator: the Monte Carlo sample ``(X, y, w)`` that
    ``mc_sample_from_gp`` returned, reweighted under ``n_draws`` joint realisations f_s of the surrogate at its rows
    (``gpry_sample_joint``).  With mu the unclipped mean the draws are centred on, log r_si = f_s(x_i) - mu(x_i),
    dlogZ_s = log sum_i w_i r_si, and mean, covariance and Kish effective sample size of the weights w_i r_si.

    More than ``max_points`` (at most 4096) rows of non-zero weight: ``max_points`` of them by systematic resampling on
    the weights (generator seeded from ``seed``), each kept row weighted by how often it was taken -- equal weights on
    the resampled rows.  Otherwise all rows with their weights.  ``seed`` is also the seed of the draws (None: fresh
    entropy).  Warns when the smallest effective sample size is below 5 % of the rows: the surrogate is then too
    uncertain for the reweighting to mean anything, which is itself the finding.  Returns a ``SurrogateSpread``;
    ``mc_sample_from_gp.last_result`` is left as it is."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    y = np.asarray(y, dtype=float)
    n, d = X.shape
    w = np.full(n, 1.0 / max(n, 1)) if w is None else np.asarray(w, dtype=float)
    if y.shape != (n,) or w.shape != (n,):
        raise ValueError(f"expected y and w of shape ({n},), got {y.shape} and {w.shape}")
    n_draws, max_points = int(n_draws), int(max_points)
    if n_draws < 2:
        raise ValueError(f"n_draws must be at least 2 (got {n_draws})")
    if not 1 <= max_points <= gpr.JOINT_MAX_POINTS:
        raise ValueError(f"max_points must lie in [1, {gpr.JOINT_MAX_POINTS}] (got {max_points})")
    if seed is None:
        seed = int(np.random.default_rng().integers(2**63 - 1))
    seed = int(seed)
    keep = np.flatnonzero((w > 0) & np.isfinite(w) & np.isfinite(y))
    if len(keep) == 0:
        raise ValueError("the sample has no row of positive weight and finite y")
    wk = w[keep] / w[keep].sum()
    if len(keep) > max_points:
        idx, counts = np.unique(_systematic(wk, max_points, np.random.default_rng(seed)), return_counts=True)
        keep, wk = keep[idx], counts / counts.sum()
    Xk, yk = np.ascontiguousarray(X[keep]), y[keep]
    m = len(keep)
    gpr._ensure_factor()
    gpr._push_affine()
    gpr.n_eval += m
    # a row whose mean sits at the clip has lost mu: there f_s - mu is taken from the variates and the factor instead
    clip = gpr._clip_hi()
    clipped = bool(np.isfinite(clip) and np.any(yk >= clip))
    res = gpr.device.sample_joint(Xk, n_draws, seed, jitter=jitter, mask=gpr._joint_mask(Xk, False, False),
                                  want_Z=clipped, want_Lc=clipped)
    with np.errstate(invalid="ignore"):
        logr = res["Z"] @ res["Lc"].T if clipped else res["Y"] - res["mean"][None, :]
    logr[~np.isfinite(res["Y"])] = -np.inf            # rows the gates reject take no part
    a = np.log(wk)[None, :] + logr
    top = a.max(axis=1)
    if not np.all(np.isfinite(top)):
        raise ValueError("every row of the sample is rejected by the classifier or the trust region")
    e = np.exp(a - top[:, None])
    tot = e.sum(axis=1)
    dlogZ = top + np.log(tot)
    ws = e / tot[:, None]
    ess = 1.0 / np.sum(ws * ws, axis=1)
    means = ws @ Xk
    cen = Xk[None, :, :] - means[:, None, :]
    covs = np.einsum("si,sia,sib->sab", ws, cen, cen)
    mean0 = wk @ Xk
    cov0 = np.einsum("i,ia,ib->ab", wk, Xk - mean0, Xk - mean0)
    var0 = np.diag(cov0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_shift_sigma = means.std(axis=0) / np.sqrt(var0)
        cov_ratio_std = (np.einsum("saa->sa", covs) / var0).std(axis=0)
    out = SurrogateSpread(dlogZ=dlogZ, means=means, covs=covs, ess=ess, mean0=mean0, cov0=cov0,
                          logZ_std=float(dlogZ.std()), mean_shift_sigma=mean_shift_sigma, cov_ratio_std=cov_ratio_std,
                          ess_min=float(ess.min()), jitter_used=res["jitter_used"], n_points=m,
                          device_ms=res["device_ms"], seed=seed)
    if out.ess_min < 0.05 * m:
        warnings.warn(f"surrogate_spread: the smallest effective sample size over the draws is {out.ess_min:.1f} of {m} "
                      "rows (< 5 %): the surrogate is too uncertain for the reweighted sample to mean anything")
    return out


class GPValidation:
    """What ``validate_gp`` returns.  ``loo`` and ``seq`` (leave-one-out, one-step-ahead) each hold ``z`` (n,; the
    z-scores (y - mean) / sqrt(var_y)), ``rms`` (of z; 1 for a calibrated model), ``frac1`` / ``frac2`` (the fractions
    with |z| <= 1 and |z| <= 2; ``GAUSS1`` = 0.683 and ``GAUSS2`` = 0.954 for a Gaussian), ``mean_logpdf`` (the mean log
    predictive density of the observations) and ``outliers`` (the indices with |z| > 3).  With groups: ``groups`` holds
    ``chi2``, ``dof``, ``logpdf``, ``info`` (one per group) and ``indices``.  ``n`` and ``device_ms``."""
    GAUSS1, GAUSS2 = 0.6826894921370859, 0.9544997361036416

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        part = "; ".join(f"{k}: rms z {v['rms']:.3g}, |z|<=1 {v['frac1']:.3f}, |z|<=2 {v['frac2']:.3f}, "
                         f"{len(v['outliers'])} beyond 3" for k, v in (("loo", self.loo), ("seq", self.seq)))
        return f"GPValidation(n={self.n}; {part})"


def _z_report(y, mean, var):
    z = (y - mean) / np.sqrt(var)
    a = np.abs(z)
    return dict(z=z, rms=float(np.sqrt(np.mean(z * z))), frac1=float(np.mean(a <= 1.0)), frac2=float(np.mean(a <= 2.0)),
                mean_logpdf=float(np.mean(-0.5 * z * z - 0.5 * np.log(2.0 * np.pi * var))),
                outliers=np.flatnonzero(a > 3.0))


def validate_gp(gpr, groups=None):
    """Cross-validation of the surrogate against the training set it already holds (Rasmussen & Williams 5.4.2): no
    likelihood call and no refit, from the factor on the device (``gpr.loo``, ``gpr.leave_out``), at the current
    hyper-parameters and pre-processors.  Leave-one-out asks whether each point is predicted by all the others;
    one-step-ahead whether it was predicted by the points acquired before it (its log densities sum to the log marginal
    likelihood); ``groups`` (index sequences into ``X_train``, or ``"last"``) whether each batch as a whole was
    predicted by the rest -- the points of a Kriging-believer batch are correlated, so their z-scores are not
    independent and chi^2 with n_g degrees of freedom is the statistic.  A pure report: it warns of nothing and changes
    nothing.  Returns a ``GPValidation``."""
    res = gpr.loo()
    y = np.asarray(gpr.y_train, dtype=float)
    out = dict(n=len(y), loo=_z_report(y, res["mean"], res["var_y"]), seq=_z_report(y, res["seq_mean"], res["seq_var_y"]),
               groups=None, device_ms=res["device_ms"])
    if groups is not None:
        g = gpr.leave_out(groups)
        out["groups"] = dict(chi2=g["chi2"], dof=g["dof"], logpdf=g["logpdf"], info=g["info"], indices=g["groups"])
        out["device_ms"] += g["device_ms"]
    return GPValidation(**out)


class BatchInfluence:
    """What ``batch_influence`` returns.  Per group g (arrays of length ``len(groups)``), "before" being the surrogate
    without the group's training points and "now" the one the regressor holds: ``dlogZ`` (log Z_before - log Z_now),
    ``kl`` (the Kullback-Leibler divergence from the posterior now to the posterior before, >= 0), ``ess`` (Kish, of the
    sample reweighted to "before"), ``means`` (ngroups, d) and ``covs`` (ngroups, d, d) of the reweighted sample,
    ``mean_shift_sigma`` (ngroups, d; |mean_before - mean_now| in units of today's posterior sigma), ``cov_ratio``
    (ngroups, d; variance before over variance now), ``max_abs_logr``, ``var_gain`` (the latent variance the group
    removed, averaged over the posterior now) and ``info`` (non-zero: the group's block of K^-1 is not positive definite,
    its entries are NaN).  ``mean0`` / ``cov0``: today's moments.  ``groups`` (the index arrays), ``keep`` (the sample rows
    that took part), ``n_points``, ``device_ms`` and, with ``groups="each"``, ``order``: the training indices by
    descending ``kl``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"BatchInfluence(n_points={self.n_points}, n_groups={len(self.dlogZ)}, "
                f"kl_max={float(np.nanmax(self.kl)):.3g}, ess_min={float(np.nanmin(self.ess)):.1f})")


def batch_influence(gpr, X, y, w=None, groups="last"):
    """What a group of training points bought: the Monte Carlo sample ``(X, y, w)`` of today's surrogate (as
    ``mc_sample_from_gp`` returns it) reweighted under the surrogate WITHOUT the group, from the factor on the device
    (``gpr.predict_without``): no second sample, no Gaussian approximation, no refit and no likelihood call.  With
    log r_i = mean_without(x_i) - mean(x_i), per group: dlogZ = log sum_i w_i r_i, kl = -sum_i w_i log r_i + dlogZ (the
    quantity the ``GaussianKL`` convergence criterion of the reference estimates from two Gaussian fits), and the moments and
    Kish effective sample size of the weights w_i r_i.  ``groups``: as for ``gpr.predict_without``; ``"last"`` asks what
    the last ``append_to_data`` changed, ``"each"`` is the jackknife over the training points (case-deletion influence
    of every likelihood evaluation, ``order`` sorting them).  The rows that take part are those of positive finite
    weight and finite y.  The counterfactual is at today's hyper-parameters and pre-processors, unclipped and ungated.
    Warns when a group's effective sample size is below 5 % of the rows.  A report: it changes nothing.  Returns a
    ``BatchInfluence``."""
    X = np.atleast_2d(np.asarray(X, dtype=float))
    y = np.asarray(y, dtype=float)
    n, d = X.shape
    w = np.full(n, 1.0 / max(n, 1)) if w is None else np.asarray(w, dtype=float)
    if y.shape != (n,) or w.shape != (n,):
        raise ValueError(f"expected y and w of shape ({n},), got {y.shape} and {w.shape}")
    keep = np.flatnonzero((w > 0) & np.isfinite(w) & np.isfinite(y))
    if len(keep) == 0:
        raise ValueError("the sample has no row of positive weight and finite y")
    wk = w[keep] / w[keep].sum()
    Xk = np.ascontiguousarray(X[keep])
    m = len(keep)
    each = isinstance(groups, str) and groups == "each"
    res = gpr.predict_without(Xk, groups)
    info = np.asarray(res["info"])
    ok = info == 0
    ng = len(info)
    logr = np.asarray(res["dmean"], dtype=float)[ok]
    dlogZ, ws, ess, means, covs, mean0, cov0 = _reweight(wk, Xk, logr)
    kl = dlogZ - logr.dot(wk)
    var0 = np.diag(cov0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_shift_sigma = np.abs(means - mean0[None, :]) / np.sqrt(var0)
        cov_ratio = np.einsum("saa->sa", covs) / var0
    max_abs_logr = np.max(np.abs(logr), axis=1) if len(logr) else np.zeros(0)
    var_gain = np.asarray(res["dvar"], dtype=float)[ok].dot(wk)

    def spread(a):                                      # the per-group arrays keep their length: NaN where info != 0
        full = np.full((ng,) + a.shape[1:], np.nan)
        full[ok] = a
        return full
    out = dict(dlogZ=spread(dlogZ), kl=spread(kl), ess=spread(ess), means=spread(means), covs=spread(covs),
               mean_shift_sigma=spread(mean_shift_sigma), cov_ratio=spread(cov_ratio), max_abs_logr=spread(max_abs_logr),
               var_gain=spread(var_gain), mean0=mean0, cov0=cov0, info=info, groups=res["groups"], keep=keep, n_points=m,
               device_ms=res["device_ms"])
    if each:
        out["order"] = np.argsort(-np.where(np.isnan(out["kl"]), -np.inf, out["kl"]), kind="stable")
    out = BatchInfluence(**out)
    if len(ess) and ess.min() < 0.05 * m:
        warnings.warn(f"batch_influence: the smallest effective sample size over the groups is {ess.min():.1f} of {m} "
                      "rows (< 5 %): the surrogate without that group is too far from today's for the reweighted sample to "
                      "mean anything")
    return out


def mc_sample_from_gp_ns(gpr, bounds=None, params=None, sampler=None, sampler_options=None, output=None, run=True,
                         verbose=3, seed=None):
    """gpry/mc.py:328-456 with the device nested sampler in place of PolyChord / UltraNest: ``(X, y, w)``.  ``sampler``
    may be None, "nested", "polychord" or "ultranest" (all run the device sampler; their options are PolyChord's);
    ``run=False`` has no initialised sampler object to return and raises."""
    if not run:
        raise ValueError("run=False returns an initialised PolyChord / UltraNest sampler in the reference; the device "
                         "nested sampler has no such object: call with run=True")
    if sampler is not None and (not isinstance(sampler, str)
                                or sampler.lower() not in ("nested", "polychord", "ultranest")):
        raise ValueError(f"Nested sampler {sampler!r} unknown: the device sampler stands for 'nested', 'polychord' "
                         "and 'ultranest'")
    return mc_sample_from_gp(gpr, bounds=bounds, sampler="nested", sampler_options=sampler_options, output=output,
                             seed=seed, params=params)
