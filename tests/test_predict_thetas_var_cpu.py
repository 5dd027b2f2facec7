"""The predictive variance under a batch of thetas without a GPU: the host side of ``gpry_predict_thetas_var`` on the
stand-in device of tests/tools/predict_thetas_var_model.py -- ``gpr.predict_thetas(return_std=True)`` and ``hyper_predict``
(the total-variance identity, row 0, failed draws, the draws of ``hyper_spread``, the weights, the fitted model untouched).
"""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict_thetas_model as pm  # noqa: E402
import predict_thetas_var_model as vm  # noqa: E402
import theta_grad_model as tm  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd.kernels import RBF, ConstantKernel as C, WhiteKernel  # noqa: E402

BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0]])
L_BOUNDS = [1e-3, 10.0]


def data(n=36, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


def make_gpr(kernel=None, device=None):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    kernel = C(1.5, [1e-3, 1e4]) * RBF([0.4, 0.7], L_BOUNDS) + WhiteKernel(1e-2, [1e-6, 1e1]) if kernel is None else kernel
    gpr = attach(GaussianProcessRegressor(kernel=kernel, bounds=BOUNDS, n_restarts_optimizer=1, noise_level=1e-2,
                                          preprocessing_X=Normalize_bounds(BOUNDS), preprocessing_y=Normalize_y(),
                                          account_for_inf=None, random_state=3),
                 vm.PredictThetasVarDevice() if device is None else device)
    gpr.fit_lockstep = False
    gpr.append_to_data(*data(), fit_gpr=False)
    return gpr


def laplace_with(gpr, cov_diag):
    """The report of the model with a covariance put in by hand (test_predict_thetas_cpu.py's)."""
    from gpry_amd.mc import hyper_laplace
    lap = hyper_laplace(gpr)
    p = len(lap.theta)
    rng = np.random.default_rng(2)
    A = rng.standard_normal((p, p)) * 0.2 + np.eye(p)
    return lap._replace(negdef=True, free=np.ones(p, dtype=bool), cov=cov_diag * A.dot(A.T))


def points(n=30, seed=9):
    return np.random.default_rng(seed).uniform(0, 1, (n, 2))


# ------------------------------------------------------------------------------------ the stand-in and the reference
@pytest.mark.parametrize("case", [(50, 1, 1, False), (130, 2, 3, True)])
def test_the_two_numpy_formulations_agree_and_the_stand_in_is_formulation_a(case):
    N, d, kid, white = case
    dev = vm.PredictThetasVarDevice()
    X_, y_, a, th = tm.load(dev, case)
    Xq_ = tm.points(case, X_)
    T = pm.thetas_of(case, th)
    Xq = tm.to_raw(case, Xq_)
    out = dev.predict_thetas(T, Xq, want_var=True)
    plain = dev.predict_thetas(T, Xq)
    assert "var" not in plain and all(np.array_equal(out[k], plain[k]) for k in ("mean", "lml", "info"))
    for b in range(5):
        va = vm.var_numpy(X_, a, T[b], kid, white, Xq_, tm.Y_STD)
        vb = vm.var_via_V(X_, a, T[b], kid, white, Xq_, tm.Y_STD)
        prior = tm.Y_STD * tm.Y_STD * vm.prior_var(T[b], d, white)
        # (cond(K) 1e4 .. 2e6 times the rounding of float64, of the prior variance the difference is taken from)
        assert np.max(np.abs(va - vb)) <= 1e-9 * prior
        assert np.max(np.abs(out["var"][b] - va)) <= 1e-12 * prior
        assert np.all(out["var"][b, -2:] == prior)                      # far outside: the prior variance exactly
        assert np.all(va[:8] < 0.5 * prior)                             # at training rows the data explain most of it
    one = dev.predict_thetas(T[3:4], Xq[5:6], want_var=True)
    assert one["var"][0, 0] == out["var"][3, 5]
    assert np.array_equal(dev.theta_full, th) and dev._factor is not None


# ------------------------------------------------------------------------------------ gpr.predict_thetas
def test_return_std_adds_the_std_and_the_default_is_the_three_tuple():
    X = points()
    gpr = make_gpr()
    th = gpr.kernel_.theta.copy()
    T = np.vstack([th, th + 0.3 * np.random.default_rng(1).standard_normal((3, 4))])
    before = gpr.predict(X, return_std=True)
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    plain = gpr.predict_thetas(X, T)
    assert len(plain) == 3 and gpr._dev.n_ptv == 0
    got = gpr.predict_thetas(X, T, return_std=True)
    assert len(got) == 4 and gpr._dev.n_ptv == 1
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 2 * 4 * 30, l0 + 2 * 4)
    mean, std, lml, info = got
    assert mean.shape == (4, 30) and std.shape == (4, 30) and lml.shape == (4,) and info.shape == (4,)
    assert np.array_equal(mean, plain[0]) and np.array_equal(lml, plain[1]) and np.array_equal(info, plain[2])
    dev = gpr._dev
    for b in range(4):
        want = np.sqrt(np.maximum(vm.var_numpy(dev.X_, dev.alpha, T[b], 0, True, dev._to_unit(X), dev.y_std), 0.0))
        assert np.allclose(std[b], want, rtol=0, atol=1e-12 * np.max(want))
    # row 0 is the fitted theta: the model's own std (which includes the white term)
    assert np.allclose(mean[0], before[0], rtol=0, atol=1e-12) and np.allclose(std[0], before[1], rtol=0, atol=1e-10 * np.max(std[0]))
    assert np.array_equal(gpr.predict_thetas(X, T, full=True, return_std=True)[1], std)
    # nothing moved
    after = gpr.predict(X, return_std=True)
    assert np.array_equal(gpr.kernel_.theta, th) and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert gpr._dev.n_factorize == 1


def test_a_device_with_the_two_argument_signature_still_serves_the_default_call():
    gpr = make_gpr(device=pm.PredictThetasDevice())
    X = points(7)
    T = np.vstack([gpr.kernel_.theta, gpr.kernel_.theta + 0.1])
    mean, lml, info = gpr.predict_thetas(X, T)
    assert mean.shape == (2, 7) and gpr._dev.n_pt == 1
    with pytest.raises(TypeError):
        gpr.predict_thetas(X, T, return_std=True)


def test_a_theta_that_is_not_positive_definite_has_a_nan_row_in_the_std_as_well(monkeypatch):
    gpr = make_gpr()
    X = points(9)
    T = np.vstack([gpr.kernel_.theta, gpr.kernel_.theta + 0.1, gpr.kernel_.theta - 0.1])
    real = gpr._dev.predict_thetas

    def failing(thetas, Xq, want_var=False):
        out = real(thetas, Xq, want_var=want_var)
        out["mean"][1], out["lml"][1], out["info"][1] = np.nan, -np.inf, 3
        if want_var:
            out["var"][1] = np.nan
        return out
    whole = gpr.predict_thetas(X, T, return_std=True)
    monkeypatch.setattr(gpr._dev, "predict_thetas", failing)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean, std, lml, info = gpr.predict_thetas(X, T, return_std=True)
    assert info[1] == 3 and np.isnan(std[1]).all() and np.isnan(mean[1]).all() and np.isneginf(lml[1])
    assert np.array_equal(std[[0, 2]], whole[1][[0, 2]]) and np.isfinite(std[[0, 2]]).all()
    # a variance that rounding left below zero is a std of zero, not a NaN
    monkeypatch.setattr(gpr._dev, "predict_thetas", lambda t, x, want_var=False: dict(real(t, x, want_var=True), var=np.full((3, 9), -1e-18)))
    assert np.all(gpr.predict_thetas(X, T, return_std=True)[1] == 0.0)


# ------------------------------------------------------------------------------------ hyper_predict
def test_hyper_predict_is_the_law_of_total_variance_over_the_draws_of_hyper_spread():
    from gpry_amd.mc import hyper_predict, hyper_spread
    gpr = make_gpr()
    X = points()
    lap = laplace_with(gpr, 0.02)
    th0 = gpr.kernel_.theta.copy()
    fitted = (gpr.kernel_.theta.copy(), gpr.predict(X, return_std=True), gpr.log_marginal_likelihood_value_, gpr.alpha_.copy(),
              gpr.V_.copy() if getattr(gpr, "V_", None) is not None else None)
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    r = hyper_predict(gpr, X, n_draws=12, seed=4, laplace=lap, scale=1.5)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 13 * 30, l0 + 13) and gpr._dev.n_ptv == 1
    assert r.weighted is False and not r.failed.any() and r.means.shape == (12, 30) and r.vars.shape == (12, 30)
    # the same draws as hyper_spread from the same seed
    ys = gpr.predict(X)
    spread = hyper_spread(gpr, X, ys, None, n_draws=12, seed=4, laplace=lap, scale=1.5, exact=True)
    assert np.array_equal(r.dtheta, spread.dtheta) and np.array_equal(r.lml, spread.lml) and r.lml0 == spread.lml0
    assert np.array_equal(r.theta_logw, spread.theta_logw) and r.theta_ess == spread.theta_ess
    assert np.allclose(r.sigma_theta, spread.sigma_theta_draws, rtol=1e-12)
    # the per-draw arrays are the refactorised model's, the summaries the mixture's moments written out
    dev = gpr._dev
    Xu = dev._to_unit(X)
    for s in (0, 5, 11):
        th = th0 + r.dtheta[s]
        assert np.allclose(r.means[s], tm.mean_numpy(dev.X_, dev.y_, dev.alpha, th, 0, True, Xu, dev.y_mean, dev.y_std), rtol=0, atol=1e-12)
        assert np.allclose(r.vars[s], vm.var_numpy(dev.X_, dev.alpha, th, 0, True, Xu, dev.y_std), rtol=0, atol=1e-12)
    v = np.maximum(r.vars, 0.0)
    second = np.mean(v + r.means ** 2, axis=0)                          # E[y^2] of the equal-weight mixture
    total = second - r.means.mean(axis=0) ** 2
    assert np.allclose(r.mean, r.means.mean(axis=0), rtol=1e-13)
    assert np.allclose(r.sigma_total ** 2, total, rtol=0, atol=1e-12 * np.max(second))
    assert np.allclose(r.sigma_gp ** 2, v.mean(axis=0), rtol=1e-13) and np.allclose(r.sigma_theta, r.means.std(axis=0), rtol=1e-12)
    assert np.allclose(r.sigma_total ** 2, r.sigma_gp ** 2 + r.sigma_theta ** 2, rtol=1e-14)
    assert np.all(r.sigma_total >= r.sigma_gp) and np.any(r.sigma_theta > 0)
    assert np.array_equal(r.inflation, r.sigma_total / r.sigma0)
    # row 0: the model's own predict(return_std=True), clip off
    assert np.allclose(r.mean0, fitted[1][0], rtol=0, atol=1e-12) and np.allclose(r.sigma0, fitted[1][1], rtol=0, atol=1e-10 * np.max(r.sigma0))
    # reproducible; and the fitted regressor is bit for bit where it was
    again = hyper_predict(gpr, X, n_draws=12, seed=4, laplace=lap, scale=1.5)
    for name in ("mean0", "sigma0", "mean", "sigma_gp", "sigma_theta", "sigma_total", "inflation", "means", "vars", "lml", "theta_logw"):
        assert np.array_equal(getattr(r, name), getattr(again, name)), name
    after = gpr.predict(X, return_std=True)
    assert np.array_equal(gpr.kernel_.theta, fitted[0]) and np.array_equal(after[0], fitted[1][0]) and np.array_equal(after[1], fitted[1][1])
    assert gpr.log_marginal_likelihood_value_ == fitted[2] and np.array_equal(gpr.alpha_, fitted[3])
    assert gpr._dev.n_factorize == 1 and np.array_equal(gpr._dev.theta_full, th0)


def test_failed_draws_take_no_part_and_all_failed_raises(monkeypatch):
    from gpry_amd.mc import hyper_predict
    gpr = make_gpr()
    X = points(20)
    lap = laplace_with(gpr, 0.02)
    real = gpr._dev.predict_thetas
    fail = {"rows": [3, 7]}

    def failing(thetas, Xq, want_var=False):
        out = real(thetas, Xq, want_var=want_var)
        for b in fail["rows"]:
            out["mean"][b], out["lml"][b], out["info"][b] = np.nan, -np.inf, 2
            if want_var:
                out["var"][b] = np.nan
        return out
    whole = hyper_predict(gpr, X, n_draws=10, seed=2, laplace=lap)
    monkeypatch.setattr(gpr._dev, "predict_thetas", failing)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # no NaN reaches a sum
        r = hyper_predict(gpr, X, n_draws=10, seed=2, laplace=lap)
    good = [s for s in range(10) if s + 1 not in fail["rows"]]
    assert np.array_equal(np.flatnonzero(r.failed), [2, 6])
    assert np.isnan(r.means[r.failed]).all() and np.isnan(r.vars[r.failed]).all() and np.all(np.isneginf(r.theta_logw[r.failed]))
    assert np.array_equal(r.means[good], whole.means[good]) and np.array_equal(r.vars[good], whole.vars[good])
    assert np.allclose(r.mean, whole.means[good].mean(axis=0), rtol=1e-13)
    assert np.allclose(r.sigma_gp ** 2, np.maximum(whole.vars[good], 0.0).mean(axis=0), rtol=1e-13)
    assert np.allclose(r.sigma_theta, whole.means[good].std(axis=0), rtol=1e-12)
    assert np.isfinite(r.sigma_total).all() and np.isfinite(r.inflation).all()
    for weighted in (False, True):
        fail["rows"] = list(range(1, 11))
        with pytest.raises(ValueError, match="not positive definite at any"):
            hyper_predict(gpr, X, n_draws=10, seed=2, laplace=lap, weighted=weighted)
        fail["rows"] = [0]
        with pytest.raises(ValueError, match="theta itself"):
            hyper_predict(gpr, X, n_draws=10, seed=2, laplace=lap, weighted=weighted)


def test_weighted_with_equal_weights_is_the_unweighted_answer_and_unequal_weights_are_applied():
    from gpry_amd.mc import hyper_predict
    gpr = make_gpr()
    X = points(20)
    lap = laplace_with(gpr, 0.05)
    th0 = np.asarray(lap.theta)
    P = np.linalg.inv(lap.cov)
    # a log marginal likelihood that IS the Laplace Gaussian: theta_logw = 0 at every draw
    gpr._dev.lml_fn = lambda th: -7.5 - 0.5 * (th - th0).dot(P).dot(th - th0)
    plain = hyper_predict(gpr, X, n_draws=16, seed=8, laplace=lap)
    w = hyper_predict(gpr, X, n_draws=16, seed=8, laplace=lap, weighted=True)
    assert w.weighted is True and np.max(np.abs(w.theta_logw)) <= 1e-12 * np.max(np.abs(w.lml - w.lml0))
    assert abs(w.theta_ess - 16.0) <= 1e-9 and abs(plain.theta_ess - 16.0) <= 1e-9
    for name in ("mean", "sigma_gp", "sigma_theta", "sigma_total", "inflation"):
        assert np.allclose(getattr(w, name), getattr(plain, name), rtol=1e-11, atol=0), name
    # a flat log marginal likelihood: the weights are exp(quad), written out
    gpr._dev.lml_fn = lambda th: -7.5
    r = hyper_predict(gpr, X, n_draws=16, seed=8, laplace=lap, weighted=True)
    quad = 0.5 * np.einsum("sf,fg,sg->s", r.dtheta, P, r.dtheta)
    assert np.allclose(r.theta_logw, quad, rtol=1e-12)
    wt = np.exp(quad - quad.max())
    wt /= wt.sum()
    mean = wt.dot(r.means)
    assert np.allclose(r.mean, mean, rtol=1e-12)
    assert np.allclose(r.sigma_gp ** 2, wt.dot(np.maximum(r.vars, 0.0)), rtol=1e-12)
    assert np.allclose(r.sigma_theta ** 2, wt.dot((r.means - mean) ** 2), rtol=1e-10)
    assert abs(r.theta_ess - 1.0 / np.sum(wt * wt)) <= 1e-9 * r.theta_ess and r.theta_ess < 16.0
    assert not np.allclose(r.mean, plain.mean, rtol=1e-6)
    # bounds that every draw leaves: weighted has nothing to average, unweighted keeps the draws
    bounds = np.array(lap.bounds, dtype=float)
    bounds[0] = [th0[0] + 50.0, th0[0] + 60.0]
    with pytest.raises(ValueError, match="no draw of theta has a weight"):
        hyper_predict(gpr, X, n_draws=16, seed=8, laplace=lap._replace(bounds=bounds), weighted=True)
    assert np.isfinite(hyper_predict(gpr, X, n_draws=16, seed=8, laplace=lap._replace(bounds=bounds)).sigma_total).all()


def test_hyper_predict_refuses_what_hyper_spread_refuses():
    from gpry_amd.mc import hyper_predict
    gpr = make_gpr()
    X = points(5)
    lap = laplace_with(gpr, 0.02)
    with pytest.raises(ValueError, match="n_draws"):
        hyper_predict(gpr, X, n_draws=1, laplace=lap)
    with pytest.raises(ValueError, match="scale"):
        hyper_predict(gpr, X, laplace=lap, scale=0.0)
    with pytest.raises(ValueError, match="negdef"):
        hyper_predict(gpr, X, laplace=lap._replace(negdef=False))
    with pytest.raises(ValueError, match="free"):
        hyper_predict(gpr, X, laplace=lap._replace(free=np.zeros(4, dtype=bool)))
