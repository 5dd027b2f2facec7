"""Maximum and profiles of the surrogate's posterior mean, and the maximum of the LogExp acquisition, with the ascents
run on the device.

A run ends with a weighted sample of the surrogate (``gpry_amd/mc.py``); this module adds what a user asks for next: the
surrogate's best-fit point (``maximize_gp``) and profile likelihoods over one or two parameters (``profile_gp``).  Whole
batches of constrained local maximisations run in one HIP kernel (``gpry_amd/csrc/maximize.hip``), value and gradient of
the mean evaluated inside it.  This module keeps the rest (starts, the first inverse-Hessian guess, the grid and its
continuation passes) and talks to the device through one call, so any object with the same method can stand in for it
(the CPU tests use a numpy one, tests/tools/maximize_numpy.py):

``dev.maximize_mean(lo, hi, X0, y0, fixed, H0, max_iter, max_halvings, gtol, ftol, minus_inf_value)
    -> {"X": (nstart, d), "y", "G": (nstart, d), "iters", "ncalls", "ngrad", "status", "device_ms"}``

The device's part, per start: a projected BFGS ascent in the unit cube u = (x - lo) / (hi - lo) with an Armijo
backtracking search; coordinates on a wall with the gradient pointing outward, and the ``fixed`` ones, do not move; the
objective is ``gpr.predict(x[None])`` bit for bit (a gated point is -inf and is never accepted), the gradient that of
the unclipped, ungated mean.  ``status`` is an index into ``MAX_STATUS``; the full statement is in include/gpry_hip.h
(gpry_maximize_mean).

``maximize_acq`` does the same for the LogExp acquisition a = 2 zeta (y - y_max) + log sqrt(sigma^2 - sigma_n^2), which
needs sigma and its gradient, O(N^2) per point (``gpry_amd/csrc/maximize_acq.hip``), through

``dev.maximize_acq(lo, hi, X0, fixed, H0, zeta, baseline, sigma_n, max_iter, max_halvings, gtol, ftol, minus_inf_value)
    -> {"X", "a", "y", "sigma", "G", "iters", "ncalls", "ngrad", "status", "device_ms"}``

with the same ascent and the exact gradient of a (gpry_maximize_acq in include/gpry_hip.h).
``BatchOptimizer(acq_optimizer="device")`` of gpry_amd/gp_acquisition.py runs its restarts through it.

``hessian_gp`` returns value, gradient and Hessian of the mean at a batch of points from one more kernel
(``gpry_amd/csrc/hessian.hip``, the Hessian's bulk a weighted Gram on the FP64 matrix pipe), through

``dev.hessian_mean(X) -> {"y": (npts,), "g": (npts, d), "H": (npts, d, d), "device_ms"}``

(stand-in: tests/tools/hessian_numpy.py); ``laplace_gp`` makes the Gaussian approximation at a maximum from it (covariance
and Laplace evidence), and ``covmat="laplace"`` takes the first inverse-Hessian guess of ``maximize_gp`` / ``profile_gp``
and the first proposal of the chain samplers (``mc_sample_from_gp``) from the curvature instead of the scatter of the
training set.  A Matern-1/2 model has no Hessian at its training rows and is refused by all of these.

No multi-GPU split of the starts; a start has a workgroup to itself (several starts do not share a pass over V); models
above 4096 padded rows are refused by ``maximize_acq``.
"""
import warnings
from collections import namedtuple
from time import time

import numpy as np

from gpry_amd.mcmc import _weighted_cov
from gpry_amd.nested import cholesky_ridged

MAX_STATUS = ("CONVERGED_G", "CONVERGED_F", "STALLED", "MAXITER", "BAD_START", "BAD_GRADIENT")
DISTINCT_TOL = 1e-6

MaxResult = namedtuple("MaxResult", ["x", "y", "X_all", "y_all", "G_all", "status", "iters", "ncalls", "ngrad",
                                     "n_distinct", "device_s", "wall_s"])
MaxResult.__doc__ = """Output of ``maximize_gp``.  x, y: the best end point (the largest finite y).  X_all, y_all, G_all:
every start's end point, its y and its unit-cube gradient; status (index into ``MAX_STATUS``), iters, ncalls (evaluations
of the mean), ngrad per start.  n_distinct: the end points with a finite y that lie further than 1e-6 apart in the unit
cube, i.e. the local maxima found.  device_s / wall_s: time in the device call / in the whole function."""

AcqMaxResult = namedtuple("AcqMaxResult", ["x", "acq", "y", "sigma", "X_all", "acq_all", "y_all", "sigma_all", "G_all",
                                           "status", "iters", "ncalls", "ngrad", "n_distinct", "device_s", "wall_s"])
AcqMaxResult.__doc__ = """Output of ``maximize_acq``.  x, acq, y, sigma: the best end point (the largest finite
acquisition), its acquisition, mean and standard deviation.  X_all, acq_all, y_all, sigma_all, G_all: every start's end
point, its values and the unit-cube gradient of the acquisition there; status (index into ``MAX_STATUS``), iters, ncalls
(evaluations of the acquisition), ngrad per start.  n_distinct: the end points with a finite acquisition that lie further
than 1e-6 apart in the unit cube.  device_s / wall_s: time in the device call / in the whole function."""

ProfileResult = namedtuple("ProfileResult", ["grid", "y", "X", "status", "ncalls", "device_s"])
ProfileResult.__doc__ = """Output of ``profile_gp``.  grid (G, len(params)): the fixed values; y (G,): the largest mean
with them fixed (-inf: no start of the row was usable); X (G, d): where; status (G,): the status of the start that gave
it (-1: none); ncalls: evaluations of the mean, all passes (``gpr.n_eval`` grows by it); device_s: time in the device calls."""


LaplaceResult = namedtuple("LaplaceResult", ["x", "y", "g", "H", "free", "cov", "logZ", "negdef", "device_s", "wall_s"])
LaplaceResult.__doc__ = """Output of ``laplace_gp``.  x: the point; y, g (d,), H (d, d): ``gpr.predict(x[None])`` and the
gradient and Hessian of the unclipped, ungated mean there, raw coordinates.  free (d,) bool: the coordinates the
approximation is over (not fixed, not held by a wall of the box); negdef: -H over the free set has a Cholesky factor;
cov (k, k): its inverse, None when not negdef; logZ: the Laplace evidence under the uniform prior over the box, NaN
unless every coordinate is free and negdef holds.  device_s / wall_s: time in the device calls / in the whole function."""


def _setup(gpr, bounds):
    from gpry_amd.mc import _bounds
    b = _bounds(gpr, bounds)
    if b.ndim != 2 or b.shape[1] != 2 or not np.all(b[:, 0] < b[:, 1]):
        raise ValueError(f"bounds must be (d, 2) with lo < hi, got {b!r}")
    return b, np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])


def _usable(X, y, lo, hi, minus_inf_value):
    """``mcmc._starts``' usability test: finite y above ``minus_inf_value``, inside the box; best first."""
    X, y = np.atleast_2d(np.asarray(X, dtype=float)), np.asarray(y, dtype=float).ravel()
    ok = np.isfinite(y) & (y > minus_inf_value) & np.all((X >= lo) & (X <= hi), axis=1)
    X, y = X[ok], y[ok]
    order = np.argsort(-y, kind="stable")
    return X[order], y[order]


def _refuse_matern12(gpr, d, who):
    """A Matern-1/2 mean has a kink at every training row: no Hessian.  (The stand-ins of the tests carry a ``kernel_id``.)"""
    kernel = getattr(gpr, "kernel_", None)
    kid = kernel.device_spec(d)[0] if hasattr(kernel, "device_spec") else getattr(gpr, "kernel_id", None)
    if kid is not None and (kid & 0xF) == 1:      # (the white-term flag is not part of the family)
        raise ValueError(f"{who}: the mean of a Matern-1/2 model is not differentiable at the training rows; it has no "
                         "Hessian")


def _inv_spd(A):
    """The inverse of a symmetric positive definite matrix and its log-determinant through its Cholesky factor, or None
    when it has none."""
    if not np.all(np.isfinite(A)):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    Li = np.linalg.solve(L, np.eye(len(A)))
    return Li.T @ Li, 2.0 * float(np.sum(np.log(np.diag(L))))


def _laplace_h0(gpr, Xt, span):
    """inv(-H_uu) at the best usable training point, unit-cube coordinates; None (and a warning) where -H_uu is not
    positive definite."""
    _refuse_matern12(gpr, len(span), 'covmat="laplace"')
    inv = None
    if len(Xt):
        H = hessian_gp(gpr, Xt[:1])[2][0]
        inv = _inv_spd(-H * np.outer(span, span))
    if inv is None:
        warnings.warn('covmat="laplace": minus the Hessian of the mean at the best training point is not positive '
                      "definite; the weighted covariance of the training set is used instead")
        return None
    return np.ascontiguousarray(0.5 * (inv[0] + inv[0].T))


def _h0(covmat, Xt, yt, span, gpr=None):
    d = len(span)
    if isinstance(covmat, str):
        if covmat != "laplace" or gpr is None:
            raise ValueError(f"covmat = {covmat!r}: a ({d}, {d}) matrix or None is needed"
                             + ("" if gpr is None else ', or "laplace"'))
        H0 = _laplace_h0(gpr, Xt, span)
        if H0 is not None:
            return H0
        covmat = None
    if covmat is not None:
        C = np.asarray(covmat, dtype=float)
        if C.shape != (d, d) or not np.all(np.isfinite(C)):
            raise ValueError(f"covmat must be a finite ({d}, {d}) matrix")
        H0 = C / np.outer(span, span)
        if not np.allclose(H0, H0.T) or np.min(np.linalg.eigvalsh(H0)) <= 0:
            raise ValueError("covmat must be symmetric positive definite")
        return np.ascontiguousarray(0.5 * (H0 + H0.T))
    if len(Xt) == 0:
        return np.eye(d)
    L = cholesky_ridged(np.atleast_2d(_weighted_cov(Xt, yt)) / np.outer(span, span))
    return np.ascontiguousarray(L @ L.T)


def _check_controls(max_iter, max_halvings, gtol, ftol):
    if int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError(f"max_iter = {max_iter!r} must be an int >= 0")
    if int(max_halvings) != max_halvings or int(max_halvings) < 0:
        raise ValueError(f"max_halvings = {max_halvings!r} must be an int >= 0")
    if not (np.isfinite(gtol) and gtol >= 0) or not (np.isfinite(ftol) and ftol >= 0):
        raise ValueError(f"gtol = {gtol}, ftol = {ftol} must be finite and >= 0")


def _mask(fixed, d):
    m = np.zeros(d, bool)
    if fixed is None:
        return m
    f = np.asarray(fixed)
    if f.dtype == bool:
        if f.shape != (d,):
            raise ValueError(f"a boolean fixed mask must have shape ({d},), got {f.shape}")
        return f.copy()
    f = np.atleast_1d(f)
    if f.ndim != 1 or not np.issubdtype(f.dtype, np.integer) or np.any((f < 0) | (f >= d)) or len(set(f.tolist())) != len(f):
        raise ValueError(f"fixed = {fixed!r}: distinct parameter indices in 0 .. {d - 1} or a boolean mask are needed")
    m[f] = True
    return m


def n_distinct(X, y, lo, hi, tol=DISTINCT_TOL):
    """The end points with a finite y further apart than ``tol`` in the unit cube (greedy, best first)."""
    fin = np.isfinite(y)
    U = ((X - lo) / (hi - lo))[fin][np.argsort(-y[fin], kind="stable")]
    kept = np.empty_like(U)
    n = 0
    for u in U:
        if n == 0 or np.all(np.max(np.abs(kept[:n] - u), axis=1) > tol):
            kept[n] = u
            n += 1
    return n


def maximize_gp(gpr, bounds=None, nstarts=64, starts=None, fixed=None, covmat=None, max_iter=200, max_halvings=12,
                gtol=1e-6, ftol=0.0, seed=None):
    """The maximum of the surrogate's posterior mean inside ``bounds`` (default ``gpr.trust_bounds``, else
    ``gpr.bounds``), from many local ascents on the device: a ``MaxResult``.

    Starts: the ``nstarts`` best usable training points (finite y above ``gpr.minus_inf_value``, inside the box), or the
    rows of ``starts`` when given.  fixed: indices (or a boolean mask) of the coordinates that keep their start values.
    H0, the first inverse-Hessian guess: ``covmat`` (raw coordinates) or the exp(y - y_max)-weighted covariance of the
    training set, in the unit cube; ``covmat="laplace"``: the inverse of minus the Hessian of the mean at the best usable
    training point (``hessian_gp``; where that is not positive definite: a warning, and the weighted covariance).
    gtol: bound on the unit-cube gradient over the free coordinates; ftol: stop when a
    step gains no more than ftol max(1, |y|) (0: off; the ascent then ends on gtol or when no step improves y any more,
    status STALLED).  ``seed`` is accepted for symmetry with the samplers; the algorithm has no randomness.  The
    defaults are provisional: nothing about them has been tuned on a real run yet.  ``gpr.n_eval`` grows by ``ncalls``,
    the evaluations of the mean (the gradients are counted in ``ngrad``)."""
    t_start = time()
    from gpry_amd.mc import _push_model
    b, lo, hi = _setup(gpr, bounds)
    d = len(lo)
    _check_controls(max_iter, max_halvings, gtol, ftol)
    mask = _mask(fixed, d)
    Xt, yt = _usable(gpr.X_train, gpr.y_train, lo, hi, gpr.minus_inf_value)
    if starts is not None:
        X0 = np.ascontiguousarray(np.atleast_2d(np.asarray(starts, dtype=float)))
        if X0.ndim != 2 or X0.shape[1] != d or len(X0) == 0 or not np.all(np.isfinite(X0)):
            raise ValueError(f"starts must be finite rows of dimension {d}, got shape {X0.shape}")
        if not np.all((X0 >= lo) & (X0 <= hi)):
            raise ValueError("every start must lie inside the bounds")
    else:
        if int(nstarts) != nstarts or int(nstarts) < 1:
            raise ValueError(f"nstarts = {nstarts!r}: at least one start is needed")
        if len(Xt) == 0:
            raise ValueError("no training point with a finite y inside the bounds to start from")
        X0 = np.ascontiguousarray(Xt[:int(nstarts)])
    H0 = _h0(covmat, Xt, yt, hi - lo, gpr)
    _push_model(gpr, "maximize")
    out = gpr.device.maximize_mean(lo, hi, X0, np.full(len(X0), np.nan), mask, H0, int(max_iter), int(max_halvings),
                                   float(gtol), float(ftol), gpr.minus_inf_value)
    gpr.n_eval += int(np.sum(out["ncalls"]))
    y = out["y"]
    fin = np.isfinite(y) & (y > gpr.minus_inf_value)
    if not fin.any():
        raise ValueError("no start has a finite mean above minus_inf_value")
    best = int(np.flatnonzero(fin)[np.argmax(y[fin])])
    return MaxResult(x=out["X"][best].copy(), y=float(y[best]), X_all=out["X"], y_all=y, G_all=out["G"],
                     status=out["status"], iters=out["iters"], ncalls=out["ncalls"], ngrad=out["ngrad"],
                     n_distinct=n_distinct(out["X"], np.where(fin, y, np.nan), lo, hi), device_s=out["device_ms"] / 1e3,
                     wall_s=time() - t_start)


def profile_gp(gpr, params, grid, bounds=None, nstarts=16, continuation=1, covmat=None, max_iter=200, max_halvings=12,
               gtol=1e-6, ftol=0.0):
    """Profile of the surrogate's posterior mean over the parameters ``params`` (one index or a tuple of indices):
    for every row of ``grid`` ((G,) or (G, len(params)); every value inside the bounds) the maximum of the mean over
    the other coordinates: a ``ProfileResult``.

    For every grid row the starts are the ``nstarts`` best usable training points with the fixed coordinates overwritten
    by the row's values; all G nstarts ascents go through one device call (one mask serves them all).  Then
    ``continuation`` passes: every row is restarted from the optima of its two neighbours in grid order, their fixed
    coordinates overwritten, and the better result is kept, which removes the jumps between branches that independent
    maximisations leave.  The other arguments and the remark on the defaults are ``maximize_gp``'s."""
    from gpry_amd.mc import _push_model
    b, lo, hi = _setup(gpr, bounds)
    d = len(lo)
    _check_controls(max_iter, max_halvings, gtol, ftol)
    par = np.atleast_1d(np.asarray(params))
    if par.ndim != 1 or len(par) == 0 or not np.issubdtype(par.dtype, np.integer):
        raise ValueError(f"params = {params!r}: one index or a tuple of indices is needed")
    mask = _mask(par, d)
    grid = np.asarray(grid, dtype=float)
    if grid.ndim == 1 and len(par) == 1:
        grid = grid[:, None]
    if grid.ndim != 2 or grid.shape[1] != len(par) or len(grid) == 0:
        raise ValueError(f"grid of shape {grid.shape} does not fit {len(par)} parameter(s)")
    if not np.all(np.isfinite(grid)) or not np.all((grid >= lo[par]) & (grid <= hi[par])):
        raise ValueError("every grid value must lie inside the bounds")
    if int(nstarts) != nstarts or int(nstarts) < 1 or int(continuation) != continuation or int(continuation) < 0:
        raise ValueError(f"nstarts = {nstarts!r}, continuation = {continuation!r}")
    G, ns = len(grid), int(nstarts)
    Xt, yt = _usable(gpr.X_train, gpr.y_train, lo, hi, gpr.minus_inf_value)
    if len(Xt) == 0:
        raise ValueError("no training point with a finite y inside the bounds to start from")
    H0 = _h0(covmat, Xt, yt, hi - lo, gpr)
    _push_model(gpr, "maximize")
    ctl = (int(max_iter), int(max_halvings), float(gtol), float(ftol), gpr.minus_inf_value)
    device_ms, ncalls = 0.0, 0

    def run(X0):
        nonlocal device_ms, ncalls
        out = gpr.device.maximize_mean(lo, hi, np.ascontiguousarray(X0), np.full(len(X0), np.nan), mask, H0, *ctl)
        device_ms += out["device_ms"]
        n = int(np.sum(out["ncalls"]))
        ncalls += n
        gpr.n_eval += n
        y = np.where(np.isfinite(out["y"]) & (out["y"] > gpr.minus_inf_value), out["y"], -np.inf)
        return out["X"], y, out["status"]

    base = Xt[:ns]
    X0 = np.repeat(base[None], G, axis=0)
    X0[:, :, par] = grid[:, None, :]
    Xo, yo, so = run(X0.reshape(-1, d))
    Xo, yo, so = Xo.reshape(G, -1, d), yo.reshape(G, -1), so.reshape(G, -1)
    j = np.argmax(yo, axis=1)
    rows = np.arange(G)
    X, y, st = Xo[rows, j].copy(), yo[rows, j].copy(), so[rows, j].astype(np.int64)
    st[np.isneginf(y)] = -1
    for _ in range(int(continuation)):
        src = [(i, k) for i in range(G) for k in (i - 1, i + 1) if 0 <= k < G and np.isfinite(y[k])]
        if not src:
            break
        Xc = np.array([X[k] for _, k in src])
        Xc[:, par] = grid[[i for i, _ in src]]
        Xn, yn, sn = run(Xc)
        for r, (i, _) in enumerate(src):
            if yn[r] > y[i]:
                X[i], y[i], st[i] = Xn[r], yn[r], sn[r]
    return ProfileResult(grid=grid, y=y, X=X, status=st, ncalls=ncalls, device_s=device_ms / 1e3)


def _hessian(gpr, X, who):
    """``dev.hessian_mean`` of the rows of X with the model pushed first and the evaluations counted."""
    from gpry_amd.mc import _push_model
    X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=float)))
    d = len(np.asarray(gpr.bounds))
    if X.ndim != 2 or X.shape[1] != d or len(X) == 0 or not np.all(np.isfinite(X)):
        raise ValueError(f"{who}: finite rows of dimension {d} are needed, got shape {X.shape}")
    _refuse_matern12(gpr, d, who)
    _push_model(gpr, "hessian")
    out = gpr.device.hessian_mean(X)
    gpr.n_eval += len(X)
    return out


def hessian_gp(gpr, X):
    """``(y, g, H)`` of the surrogate's posterior mean at the rows of ``X`` (npts, d), raw coordinates, in one device
    call: y (npts,) is ``gpr.predict(x[None])`` bit for bit (clip and gates included, a gated point is -inf); g (npts, d)
    and H (npts, d, d) are the gradient and the Hessian of the unclipped, ungated mean, H symmetric to the last bit.
    A Matern-1/2 model raises a ValueError.  ``gpr.n_eval`` grows by npts."""
    out = _hessian(gpr, X, "hessian_gp")
    return out["y"], out["g"], out["H"]


def laplace_gp(gpr, x=None, bounds=None, fixed=None, **maximize_kwargs):
    """The Gaussian approximation of exp(mean) at ``x`` inside ``bounds`` (default ``gpr.trust_bounds``, else
    ``gpr.bounds``): a ``LaplaceResult``.

    x: the point; None: the best point of ``maximize_gp(gpr, bounds=bounds, fixed=fixed, **maximize_kwargs)``.  free:
    every coordinate except the ``fixed`` ones and those on a wall of the box with the gradient pointing outward
    (x_k == lo_k and g_k <= 0, or x_k == hi_k and g_k >= 0: the ascent's own rule for a coordinate that does not move).
    With H_ff the Hessian over the k free coordinates: negdef says whether -H_ff has a Cholesky factor, cov = (-H_ff)^-1
    (None when it has none), and
    logZ = y + (k / 2) log 2 pi - (1 / 2) log det(-H_ff) - sum_free log(hi - lo), the evidence under the uniform prior over
    the box (the nested sampler's convention), NaN unless all d coordinates are free and negdef holds.  A Matern-1/2
    model raises a ValueError."""
    t_start = time()
    b, lo, hi = _setup(gpr, bounds)
    d = len(lo)
    mask = _mask(fixed, d)
    _refuse_matern12(gpr, d, "laplace_gp")
    device_s = 0.0
    if x is None:
        r = maximize_gp(gpr, bounds=b, fixed=fixed, **maximize_kwargs)
        x, device_s = r.x, r.device_s
    else:
        if maximize_kwargs:
            raise TypeError(f"{sorted(maximize_kwargs)} are arguments of the maximisation, which a given x does not run")
        x = np.array(x, dtype=float).ravel()
        if x.shape != (d,) or not np.all(np.isfinite(x)) or not np.all((x >= lo) & (x <= hi)):
            raise ValueError(f"x must be a finite point of dimension {d} inside the bounds, got {x!r}")
    out = _hessian(gpr, x[None], "laplace_gp")
    device_s += out["device_ms"] / 1e3
    y, g, H = float(out["y"][0]), out["g"][0], out["H"][0]
    free = ~mask & ~((x == lo) & (g <= 0)) & ~((x == hi) & (g >= 0))
    k = int(free.sum())
    inv = _inv_spd(-H[np.ix_(free, free)]) if k else (np.zeros((0, 0)), 0.0)
    negdef = inv is not None
    logZ = np.nan
    if negdef and k == d:
        logZ = y + 0.5 * k * np.log(2.0 * np.pi) - 0.5 * inv[1] - float(np.sum(np.log(hi - lo)))
    return LaplaceResult(x=x, y=y, g=g, H=H, free=free, cov=inv[0] if negdef else None, logZ=float(logZ), negdef=negdef,
                         device_s=device_s, wall_s=time() - t_start)


def laplace_covmat(gpr, bounds, covmat="laplace"):
    """The first proposal covariance of a chain sampler for ``covmat="laplace"``: ``laplace_gp``'s cov at the maximum
    of the mean, or None (and a warning: the sampler then starts from the weighted covariance of the training set)
    unless every coordinate is free there and negdef holds.  Any other string raises a ValueError."""
    if covmat != "laplace":
        raise ValueError(f'covmat = {covmat!r}: a matrix, None or "laplace" is needed')
    r = laplace_gp(gpr, bounds=bounds)
    if r.negdef and r.free.all():
        return r.cov
    warnings.warn('covmat="laplace": the maximum of the mean ' +
                  ("lies on a wall of the box" if not r.free.all() else "has a Hessian that is not negative definite") +
                  "; the weighted covariance of the training set is used instead")
    return None


def acq_parameters(acq_func, gpr, d):
    """``(zeta, sigma_n)`` of the acquisition function for the device ascent: a ``LogExp`` (None: ``LogExp(dimension=d)``)
    with a scalar noise level.  Anything else raises a ValueError that says so."""
    from collections.abc import Iterable
    from gpry_amd.acquisition_functions import LogExp
    if acq_func is None:
        acq_func = LogExp(dimension=d)
    if type(acq_func) is not LogExp:
        raise ValueError(f"the device ascent of the acquisition function supports gpry_amd.acquisition_functions.LogExp "
                         f"only, got {acq_func!r}")
    sigma_n = acq_func._noise(gpr)[1]
    if isinstance(sigma_n, Iterable) or not np.isfinite(sigma_n) or sigma_n < 0:
        raise ValueError("the device ascent of the acquisition function needs one scalar noise level >= 0 (give LogExp a "
                         f"sigma_n, or the regressor a scalar noise_level), got {sigma_n!r}")
    zeta = float(acq_func.zeta)
    if not np.isfinite(zeta):
        raise ValueError(f"zeta = {zeta}")
    return zeta, float(sigma_n)


def acq_h0(gpr, covmat, lo, hi):
    """The first inverse-Hessian guess of ``maximize_acq`` in the unit cube: ``covmat`` (raw coordinates) as in
    ``maximize_gp``, else diag((l_k / (hi_k - lo_k))^2) with l the kernel's length scales in raw coordinates (the identity
    for a regressor without a kernel_)."""
    d, span = len(lo), hi - lo
    if covmat is not None:
        return _h0(covmat, np.empty((0, d)), np.empty(0), span)
    kernel = getattr(gpr, "kernel_", None)
    if kernel is None:
        return np.eye(d)
    theta = np.asarray(kernel.theta, dtype=float)
    if getattr(gpr, "has_white_term", False):       # C * k + WhiteKernel: the length scales of k, wherever log w sits in theta
        theta = np.asarray(kernel._parts()[0].theta, dtype=float)
    ls = np.broadcast_to(np.exp(theta[1:]), (d,)).copy()
    px = getattr(gpr, "preprocessing_X", None)
    if px is not None and hasattr(px, "transform_bounds"):
        tb = np.asarray(px.transform_bounds(np.stack([lo, hi], axis=1)), dtype=float)
        ls = ls * span / (tb[:, 1] - tb[:, 0])
    return np.diag((ls / span) ** 2)


def maximize_acq(gpr, acq_func=None, bounds=None, starts=None, nstarts=64, fixed=None, covmat=None, max_iter=200,
                 max_halvings=12, gtol=1e-6, ftol=0.0, rng=None):
    """The maximum of the LogExp acquisition a(x) = 2 zeta (y(x) - y_max) + log sqrt(sigma(x)^2 - sigma_n^2) inside
    ``bounds`` (default ``gpr.trust_bounds``, else ``gpr.bounds``), from many local ascents on the device: an
    ``AcqMaxResult``.

    acq_func: a ``gpry_amd.acquisition_functions.LogExp`` (default ``LogExp(dimension=d)``); zeta is its own, sigma_n its
    ``_noise(gpr)`` (one scalar noise level), the baseline ``gpr.y_max``.  Anything else raises a ValueError.  Starts:
    the rows of ``starts``, or ``nstarts`` points uniform in the box drawn from ``rng`` (training rows are poor starts
    here: sigma^2 - sigma_n^2 is about 0 on them and a is -inf).  fixed, max_iter, max_halvings, gtol, ftol: as in
    ``maximize_gp``.  H0: ``covmat`` (raw coordinates), else diag((l_k / (hi_k - lo_k))^2) with l the kernel's length
    scales in raw coordinates; provisional, like the other defaults: nothing about them has been tuned on a real run.

    The device climbs with the exact gradient of a.  The reference's ``BaseLogExp.__call__`` returns
    ``std_grad / (std - sigma_n) + 2 zeta mu_grad``, the derivative of log(sigma - sigma_n) and not of the
    log sqrt(sigma^2 - sigma_n^2) that ``LogExp.f`` evaluates: its sigma term is off by the factor (sigma + sigma_n) / sigma;
    a line search needs a gradient consistent with its value, so the device does not mirror that formula.
    ``gpr.n_eval`` grows by ``ncalls``."""
    t_start = time()
    from gpry_amd.mc import _push_model
    from gpry_amd.tools import get_random_generator
    b, lo, hi = _setup(gpr, bounds)
    d = len(lo)
    _check_controls(max_iter, max_halvings, gtol, ftol)
    mask = _mask(fixed, d)
    zeta, sigma_n = acq_parameters(acq_func, gpr, d)
    if starts is not None:
        X0 = np.ascontiguousarray(np.atleast_2d(np.asarray(starts, dtype=float)))
        if X0.ndim != 2 or X0.shape[1] != d or len(X0) == 0 or not np.all(np.isfinite(X0)):
            raise ValueError(f"starts must be finite rows of dimension {d}, got shape {X0.shape}")
        if not np.all((X0 >= lo) & (X0 <= hi)):
            raise ValueError("every start must lie inside the bounds")
    else:
        if int(nstarts) != nstarts or int(nstarts) < 1:
            raise ValueError(f"nstarts = {nstarts!r}: at least one start is needed")
        X0 = np.ascontiguousarray(get_random_generator(rng).uniform(lo, hi, (int(nstarts), d)))
    H0 = acq_h0(gpr, covmat, lo, hi)
    _push_model(gpr, "maximize_acq")
    out = gpr.device.maximize_acq(lo, hi, X0, mask, H0, zeta, float(gpr.y_max), sigma_n, int(max_iter), int(max_halvings),
                                  float(gtol), float(ftol), gpr.minus_inf_value)
    gpr.n_eval += int(np.sum(out["ncalls"]))
    acq = out["a"]
    fin = np.isfinite(acq)
    if not fin.any():
        raise ValueError("no start has a finite acquisition")
    best = int(np.flatnonzero(fin)[np.argmax(acq[fin])])
    return AcqMaxResult(x=out["X"][best].copy(), acq=float(acq[best]), y=float(out["y"][best]),
                        sigma=float(out["sigma"][best]), X_all=out["X"], acq_all=acq, y_all=out["y"],
                        sigma_all=out["sigma"], G_all=out["G"], status=out["status"], iters=out["iters"],
                        ncalls=out["ncalls"], ngrad=out["ngrad"],
                        n_distinct=n_distinct(out["X"], np.where(fin, acq, np.nan), lo, hi),
                        device_s=out["device_ms"] / 1e3, wall_s=time() - t_start)
