#!/usr/bin/env python3
"""Golden vectors for kernels with a fitted noise level, ``C * (RBF | Matern) + WhiteKernel``, from the REAL reference.

Like ``tools/make_goldens.py`` (whose ``import_reference`` it reuses): runs only where the reference is mounted, drives its
public API on the CPU and writes DATA ONLY to ``tests/golden/white_noise.npz``.

    python tools/make_goldens_white.py

Per kernel id k (0 RBF, 1..3 Matern nu = 0.5, 1.5, 2.5) and shape s (0: N = 40, d = 2; 1: N = 150, d = 5), prefix ``k{k}_s{s}_``:
``bounds X y noise_level`` (raw; ``noise_level`` a scalar, per point in the case k = 2, s = 0), ``X_ y_ alpha y_mean y_std``
(transformed), ``theta`` = [log C, log l.., log w] (NOT an optimum), ``theta_bounds``, ``repr``, ``K`` = kernel_(X_) (w on
the diagonal, no alpha; at s = 1 its first sixteen rows ``K_rows`` and ``K_diag``), ``Kx`` = kernel_(Xc_, X_) (no white part), ``diag``, ``lml grad``, ``Xc mean std`` at 16 points,
``mean_grad std_grad`` (one reference call per point; not for Matern-1/2, whose x-gradient raises in the reference),
``zeta acq`` (LogExp).  ``fit_*``: a noisy data set and the reference's own fit of it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import KERNELS, OUT, REF, gauss_problem, import_reference  # noqa: E402

SHAPES = ((40, 2), (150, 5))
NOISE = 0.3


def white_kernel(kid, theta, d):
    from gpry.kernels import RBF, Matern, ConstantKernel as C, WhiteKernel
    name, kw = KERNELS[kid]
    cls = RBF if name == "RBF" else Matern
    k = C(1.0, [1e-4, 1e6]) * cls([1.0] * d, [1e-3, 10.], **kw) + WhiteKernel(1.0, [1e-6, 1e2])
    k.theta = theta
    return k


def fixed_gpr(bounds, kernel, X, y, noise_level):
    """Reference GPR at the kernel's theta (no optimiser run), as ``make_goldens.make_gpr``."""
    from sklearn.base import clone
    from gpry.gpr import GaussianProcessRegressor
    from gpry.preprocessing import Normalize_bounds, Normalize_y
    gpr = GaussianProcessRegressor(
        kernel=kernel, bounds=bounds, optimizer=None, noise_level=noise_level if not np.iterable(noise_level) else 1e-2,
        preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(), account_for_inf=None)
    gpr.kernel_ = clone(kernel)
    gpr._fitted = True
    if np.iterable(noise_level):
        # (per-point levels from the first point on: the reference's conversion of its scalar counts the new points too)
        gpr.noise_level = np.empty(0)
    gpr.append_to_data(X, y, noise_level=noise_level if np.iterable(noise_level) else None, fit_gpr=False)
    return gpr


def noisy_problem(N, d, M, seed):
    bounds, X, y, Xc = gauss_problem(N, d, M, seed)
    rng = np.random.default_rng(seed + 7)
    return bounds, X, y + NOISE * rng.standard_normal(N), Xc


def fixed_theta_cases(out):
    from gpry.acquisition_functions import LogExp
    for kid in KERNELS:
        for s, (N, d) in enumerate(SHAPES):
            p = f"k{kid}_s{s}_"
            bounds, X, y, Xc = noisy_problem(N, d, 16, seed=900 + 10 * kid + s)
            Xc[1] = X[5]                       # exactly on a training point
            per_point = kid == 2 and s == 0
            noise = np.random.default_rng(5).uniform(0.005, 0.05, N) if per_point else 1e-2
            theta = np.log(np.array([2.5] + [0.12 + 0.04 * k for k in range(d)] + [0.05]))
            gpr = fixed_gpr(bounds, white_kernel(kid, theta, d), X, y, noise)
            kern = gpr.kernel_
            lml, grad = gpr.log_marginal_likelihood(theta, eval_gradient=True)
            assert len(kern.theta) == d + 2 and grad.shape == (d + 2,)
            assert np.max(np.abs(grad)) > 1e-2 and np.min(np.abs(grad)) > 1e-6, grad     # not an optimum
            Xc_ = gpr.preprocessing_X.transform(Xc)
            out[p + "bounds"], out[p + "X"], out[p + "y"], out[p + "noise_level"] = bounds, X, y, np.asarray(noise)
            out[p + "X_"], out[p + "y_"], out[p + "alpha"] = gpr.X_train_, gpr.y_train_, np.broadcast_to(gpr.alpha, (N,)).copy()
            out[p + "y_mean"], out[p + "y_std"] = gpr.preprocessing_y.mean_, gpr.preprocessing_y.std_
            out[p + "theta"], out[p + "theta_bounds"], out[p + "repr"] = kern.theta, kern.bounds, np.array(repr(kern))
            K = kern(gpr.X_train_)
            if s == 0:
                out[p + "K"] = K
            else:                              # (N = 150: sixteen rows and the diagonal keep the file small)
                out[p + "K_rows"], out[p + "K_diag"] = K[:16].copy(), np.diag(K).copy()
            out[p + "Kx"], out[p + "diag"] = kern(Xc_, gpr.X_train_), kern.diag(Xc_)
            out[p + "lml"], out[p + "grad"] = lml, grad
            out[p + "lml_nograd"] = gpr.log_marginal_likelihood(theta)
            mean, std = gpr.predict(Xc, return_std=True)
            out[p + "Xc"], out[p + "mean"], out[p + "std"] = Xc, mean, std
            af = LogExp(dimension=d)
            out[p + "zeta"] = af.zeta
            with np.errstate(all="ignore"):
                out[p + "acq"] = af(Xc, gpr)
            if kid == 1:
                continue
            mg, sg = [], []
            for x in Xc:
                m1, s1, g1, g2 = gpr.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True)
                assert abs(m1[0] - mean[list(map(tuple, Xc)).index(tuple(x))]) < 1e-9
                mg.append(np.array(g1, dtype=float)), sg.append(np.array(g2, dtype=float))
            out[p + "mean_grad"], out[p + "std_grad"] = np.array(mg), np.array(sg)


def fitted_case(out):
    """The reference's own fit (its default number of restarts, 10 + 2 d) of N = 150 noisy points in d = 2."""
    from gpry.gpr import GaussianProcessRegressor
    from gpry.kernels import RBF, ConstantKernel as C, WhiteKernel
    from gpry.preprocessing import Normalize_bounds, Normalize_y
    N, d = 150, 2
    bounds, X, y, _ = noisy_problem(N, d, 1, seed=977)
    kernel = C(1.0, [1e-3, 1e4]) * RBF([1.0] * d, [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(
        kernel=kernel, bounds=bounds, n_restarts_optimizer=10 + 2 * d, noise_level=1e-2,
        preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(), account_for_inf=None, random_state=3)
    gpr.append_to_data(X, y, fit_gpr=True)
    w, std_y = float(np.exp(gpr.kernel_.theta[-1])), float(gpr.preprocessing_y.std_)
    target = NOISE ** 2 / std_y ** 2
    assert target / 2 < w < 2 * target, (w, target)          # the fit finds the data's noise
    out["fit_bounds"], out["fit_X"], out["fit_y"] = bounds, X, y
    out["fit_theta0"], out["fit_theta_bounds"] = kernel.theta, gpr.kernel_.bounds
    out["fit_theta"], out["fit_lml"] = gpr.kernel_.theta, gpr.log_marginal_likelihood_value_
    out["fit_y_std"], out["fit_noise_level"], out["fit_n_restarts"] = std_y, 1e-2, 10 + 2 * d
    print(f"  fitted w = {w:.4g} (0.09 / std_y^2 = {target:.4g}), lml = {out['fit_lml']:.6f}, theta = {gpr.kernel_.theta}")


def main():
    if not os.path.isdir(REF):
        print(f"{REF} not found: nothing to do")
        return 0
    version = import_reference()
    out = {}
    fixed_theta_cases(out)
    fitted_case(out)
    out["_reference_version"] = np.array(version)
    path = os.path.join(OUT, "white_noise.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
