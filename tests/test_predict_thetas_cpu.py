"""The mean under a batch of thetas without a GPU: the host side of ``gpry_predict_thetas`` on the stand-in device of
tests/tools/predict_thetas_model.py -- ``gpr.predict_thetas`` (the mapping of the kernel's entries, the counters, the shape
errors) and ``hyper_spread(exact=True)`` against a direct numpy computation from refactorised means.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict_thetas_model as pm  # noqa: E402
import theta_grad_model as tm  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd.kernels import RBF, Matern, ConstantKernel as C, WhiteKernel  # noqa: E402

BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0]])
L_BOUNDS = [1e-3, 10.0]


def data(n=36, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


def make_gpr(kernel, xy=None):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    gpr = attach(GaussianProcessRegressor(kernel=kernel, bounds=BOUNDS, n_restarts_optimizer=1, noise_level=1e-2,
                                          preprocessing_X=Normalize_bounds(BOUNDS), preprocessing_y=Normalize_y(),
                                          account_for_inf=None, random_state=3), pm.PredictThetasDevice())
    gpr.fit_lockstep = False
    gpr.append_to_data(*(data() if xy is None else xy), fit_gpr=False)
    return gpr


def white_kernel(ls=(0.4, 0.7)):
    return C(1.5, [1e-3, 1e4]) * RBF(list(ls), L_BOUNDS) + WhiteKernel(1e-2, [1e-6, 1e1])


def sample(n=200, seed=9):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (n, 2)), rng.uniform(0.5, 1.5, n)


def laplace_with(gpr, cov_diag, free=None):
    """The report of the model with a covariance put in by hand (the stand-in's model is not at an optimum)."""
    from gpry_amd.mc import hyper_laplace
    lap = hyper_laplace(gpr)
    p = len(lap.theta)
    free = np.ones(p, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    k = int(free.sum())
    rng = np.random.default_rng(2)
    A = rng.standard_normal((k, k)) * 0.2 + np.eye(k)
    return lap._replace(negdef=True, free=free, cov=cov_diag * A.dot(A.T))


def refactorised(gpr, X, theta_full, kid, white):
    """The unclipped mean at the device's vector ``theta_full``, numpy formulation (a)."""
    dev = gpr._dev
    return tm.mean_numpy(dev.X_, dev.y_, dev.alpha, theta_full, kid, white, dev._to_unit(X), dev.y_mean, dev.y_std)


def direct(dtheta, X, w, keep, logr):
    """The summaries from log r, written out (test_theta_grad_cpu.py's)."""
    wk = w[keep] / w[keep].sum()
    a = np.log(wk)[None, :] + logr
    top = a.max(axis=1)
    e = np.exp(a - top[:, None])
    tot = e.sum(axis=1)
    ws = e / tot[:, None]
    means = ws.dot(X[keep])
    cen = X[keep][None, :, :] - means[:, None, :]
    return top + np.log(tot), means, np.einsum("si,sia,sib->sab", ws, cen, cen), 1.0 / np.sum(ws * ws, axis=1)


NEW = ("lml", "lml0", "failed", "sigma_theta_draws", "first_order_miss", "theta_logw", "theta_ess")


# ------------------------------------------------------------------------------------ the stand-in and the reference
@pytest.mark.parametrize("case", [(50, 1, 1, False), (130, 2, 3, True)])
def test_the_two_numpy_formulations_agree_and_the_stand_in_is_formulation_a(case):
    N, d, kid, white = case
    dev = pm.PredictThetasDevice()
    X_, y_, a, th = tm.load(dev, case)
    Xq_ = tm.points(case, X_)
    T = pm.thetas_of(case, th)
    out = dev.predict_thetas(T, tm.to_raw(case, Xq_))
    for b in range(5):
        ma = tm.mean_numpy(X_, y_, a, T[b], kid, white, Xq_, tm.Y_MEAN, tm.Y_STD)
        mb = pm.mean_via_V(X_, y_, a, T[b], kid, white, Xq_, tm.Y_MEAN, tm.Y_STD)
        # (cond(K) 1e4 .. 2e6: the two differ by 3e-14 .. 2e-11 of the mean's range on these models)
        assert np.max(np.abs(ma - mb)) <= 1e-9 * np.max(np.abs(ma - tm.Y_MEAN))
        assert np.max(np.abs(out["mean"][b] - ma)) <= 1e-12 * np.max(np.abs(ma))
        assert out["lml"][b] == dev.lml(T[b], False)[0] and out["info"][b] == 0
    assert np.all(out["mean"][:, -2:] == tm.Y_MEAN)
    one = dev.predict_thetas(T[3:4], tm.to_raw(case, Xq_[5:6]))
    assert one["mean"][0, 0] == out["mean"][3, 5]
    # the model the device holds is not touched
    assert np.array_equal(dev.theta_full, th) and dev._factor is not None


# ------------------------------------------------------------------------------------ gpr.predict_thetas
def test_gpr_predict_thetas_maps_the_kernel_s_entries_and_changes_nothing():
    X, _ = sample(30)
    gpr = make_gpr(white_kernel())
    th = gpr.kernel_.theta.copy()
    rng = np.random.default_rng(1)
    T = np.vstack([th, th + 0.3 * rng.standard_normal((3, 4))])
    before = gpr.predict(X)
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    mean, lml, info = gpr.predict_thetas(X, T)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 4 * 30, l0 + 4) and gpr._dev.n_pt == 1
    assert mean.shape == (4, 30) and lml.shape == (4,) and not info.any()
    for b in range(4):                                  # theta is the device's own vector here
        want = refactorised(gpr, X, T[b], 0, True)
        assert np.allclose(mean[b], want, rtol=0, atol=1e-12 * np.max(np.abs(want)))
        assert lml[b] == gpr._dev.lml(T[b], False)[0]
    assert np.allclose(mean[0], before, rtol=0, atol=1e-12)
    assert np.array_equal(gpr.predict_thetas(X, T, full=True)[0], mean)
    assert np.array_equal(gpr.predict_thetas(X, T[2])[0][0], mean[2])            # one row, given as a vector
    # nothing moved
    assert np.array_equal(gpr.kernel_.theta, th) and np.array_equal(gpr.predict(X), before)
    assert gpr._dev.n_factorize == 1
    # the white term first: theta = [log w, log C, log l_1, log l_2]
    gpr = make_gpr(WhiteKernel(1e-2, [1e-6, 1e1]) + C(1.5, [1e-3, 1e4]) * RBF([0.4, 0.7], L_BOUNDS))
    th = gpr.kernel_.theta.copy()
    T = th + 0.2 * rng.standard_normal((3, 4))
    mean = gpr.predict_thetas(X, T)[0]
    for b in range(3):
        want = refactorised(gpr, X, np.append(T[b, 1:], T[b, 0]), 0, True)
        assert np.allclose(mean[b], want, rtol=0, atol=1e-12 * np.max(np.abs(want)))
    full = np.column_stack([T[:, 1:], T[:, 0]])
    assert np.array_equal(gpr.predict_thetas(X, full, full=True)[0], mean)
    assert np.array_equal(gpr.kernel_.theta, th)
    # an isotropic length scale fills both entries; a fixed constant keeps its value
    gpr = make_gpr(C(1.5, "fixed") * Matern(0.5, L_BOUNDS, nu=2.5))
    assert len(gpr.kernel_.theta) == 1
    T = np.log([[0.5], [0.3], [0.8]])
    mean = gpr.predict_thetas(X, T)[0]
    for b in range(3):
        want = refactorised(gpr, X, np.array([np.log(1.5), T[b, 0], T[b, 0]]), 3, False)
        assert np.allclose(mean[b], want, rtol=0, atol=1e-12 * np.max(np.abs(want)))
    assert gpr.predict_thetas(X, np.log([[1.5, 0.5, 0.6]]), full=True)[0].shape == (1, 30)
    assert np.array_equal(gpr.kernel_.theta, np.log([0.5]))
    # shape errors
    with pytest.raises(ValueError):
        gpr.predict_thetas(X, np.zeros((2, 2)))                     # the kernel has one entry
    with pytest.raises(ValueError):
        gpr.predict_thetas(X, np.zeros((2, 2)), full=True)          # the device's vector has three
    with pytest.raises(ValueError):
        gpr.predict_thetas(np.zeros((3, 5)), T)
    with pytest.raises(ValueError):
        gpr.predict_thetas(np.array([[0.1, np.nan]]), T)
    with pytest.raises(ValueError):
        gpr.predict_thetas(X, np.array([[np.nan]]))
    with pytest.raises(ValueError):
        gpr.predict_thetas(X, np.zeros((0, 1)))


# ------------------------------------------------------------------------------------ hyper_spread
def test_without_the_keyword_and_with_exact_false_nothing_changed():
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample()
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.02)
    a = hyper_spread(gpr, X, y, w, n_draws=16, seed=4, laplace=lap, scale=1.5)
    b = hyper_spread(gpr, X, y, w, n_draws=16, seed=4, laplace=lap, scale=1.5, exact=False)
    assert gpr._dev.n_pt == 0 and a.exact is False and b.exact is False
    for name in ("dtheta", "dlogZ", "means", "covs", "ess", "sigma_theta", "mean0", "cov0", "mean_shift_sigma", "cov_ratio_std",
                 "keep"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert (a.logZ_std, a.ess_min, a.max_abs_logr, a.n_points) == (b.logZ_std, b.ess_min, b.max_abs_logr, b.n_points)
    for name in NEW:
        assert getattr(a, name) is None and getattr(b, name) is None, name
    # ... and is the first order: log r = G . dtheta
    G = gpr.mean_theta_grad(X, full=True)[1]
    dlogZ, means, covs, ess = direct(a.dtheta, X, w, a.keep, a.dtheta.dot(G[a.keep].T))
    assert np.allclose(a.dlogZ, dlogZ, rtol=0, atol=1e-12) and np.allclose(a.means, means, rtol=0, atol=1e-13)


def test_exact_mode_equals_the_direct_computation_from_refactorised_means():
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample()
    w[:5] = 0.0
    y = gpr.predict(X)
    y[5:8] = -np.inf
    lap = laplace_with(gpr, 0.02)
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    r = hyper_spread(gpr, X, y, w, n_draws=12, seed=4, laplace=lap, scale=1.5, exact=True)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 192 + 13 * 192, l0 + 13) and gpr._dev.n_pt == 1
    first = hyper_spread(gpr, X, y, w, n_draws=12, seed=4, laplace=lap, scale=1.5)
    assert r.exact is True and np.array_equal(r.dtheta, first.dtheta) and np.array_equal(r.sigma_theta, first.sigma_theta)
    assert np.array_equal(r.keep, np.arange(8, 200)) and not r.failed.any()
    th0 = np.asarray(lap.theta)
    m0 = refactorised(gpr, X[r.keep], th0, 0, True)
    ms = np.stack([refactorised(gpr, X[r.keep], th0 + dt, 0, True) for dt in r.dtheta])
    logr = ms - m0
    dlogZ, means, covs, ess = direct(r.dtheta, X, w, r.keep, logr)
    assert np.allclose(r.dlogZ, dlogZ, rtol=1e-12, atol=1e-12 * np.max(np.abs(dlogZ)))
    assert np.allclose(r.means, means, rtol=1e-12) and np.allclose(r.ess, ess, rtol=1e-12)
    assert np.allclose(r.covs, covs, rtol=0, atol=1e-12 * np.max(np.abs(covs)))
    assert abs(r.logZ_std - dlogZ.std()) <= 1e-12 * dlogZ.std() and abs(r.ess_min - ess.min()) <= 1e-12 * ess.min()
    assert abs(r.max_abs_logr - np.max(np.abs(logr))) <= 1e-12 * np.max(np.abs(logr))
    assert np.allclose(r.sigma_theta_draws, ms.std(axis=0), rtol=1e-10)
    G = gpr.mean_theta_grad(X, full=True)[1][r.keep]
    miss = np.max(np.abs(logr - r.dtheta.dot(G.T)))
    assert r.first_order_miss > 0 and abs(r.first_order_miss - miss) <= 1e-10 * miss
    dev = gpr._dev
    lml = np.array([dev.lml(th0 + dt, False)[0] for dt in r.dtheta])
    assert np.array_equal(r.lml, lml) and r.lml0 == dev.lml(th0, False)[0]
    quad = 0.5 * np.einsum("sf,fg,sg->s", r.dtheta, np.linalg.inv(lap.cov), r.dtheta) / 1.5 ** 2
    assert np.allclose(r.theta_logw, lml - r.lml0 + quad, rtol=1e-12, atol=1e-12)
    tw = np.exp(r.theta_logw)
    assert abs(r.theta_ess - tw.sum() ** 2 / np.sum(tw * tw)) <= 1e-12 * r.theta_ess and 1.0 <= r.theta_ess <= 12.0
    # reproducible, and the model is where it was
    again = hyper_spread(gpr, X, y, w, n_draws=12, seed=4, laplace=lap, scale=1.5, exact=True)
    for name in ("dlogZ", "means", "covs", "ess", "lml", "theta_logw", "sigma_theta_draws"):
        assert np.array_equal(getattr(r, name), getattr(again, name)), name
    assert np.array_equal(gpr.kernel_.theta, th0) and gpr._dev.n_factorize == 1


def test_at_a_small_scale_the_modes_agree_to_second_order_and_at_scale_one_they_do_not():
    """(130, 2, RBF), the model of the device tests.  The remainder of the linearisation of log r is quadratic in the draw:
    at scale s it is c s^2 with c measured here at s = 1e-3 from the numpy truth itself (first_order_miss against
    ``mean_numpy``, not against the code under test); the tolerance of "the modes agree" is ten times that remainder plus the
    rounding of a difference of two means (1e-9 of their size).  At scale 1 the modes differ by far more than that tolerance:
    the test can tell them apart."""
    from gpry_amd.mc import hyper_spread
    N, d = 130, 2
    X_, y_, a, th = tm.problem(N, d, seed=N + d, white=False)
    rng = np.random.default_rng(3)
    gpr = make_gpr(C(2.0, [1e-3, 1e4]) * RBF([0.4, 0.5], L_BOUNDS), (X_, np.sin(3 * X_.sum(1)) + 0.05 * rng.standard_normal(N)))
    X, w = sample(64)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.3 ** 2)
    th0 = np.asarray(lap.theta)
    G = gpr.mean_theta_grad(X, full=True)[1]

    def truth_miss(dtheta):
        m0 = refactorised(gpr, X, th0, 0, False)
        return max(np.max(np.abs(refactorised(gpr, X, th0 + dt, 0, False) - m0 - G.dot(dt))) for dt in dtheta)
    small = hyper_spread(gpr, X, y, w, n_draws=8, seed=6, laplace=lap, scale=1e-3, exact=True)
    small1 = hyper_spread(gpr, X, y, w, n_draws=8, seed=6, laplace=lap, scale=1e-3)
    tol = 10.0 * truth_miss(small.dtheta) + 1e-9 * np.max(np.abs(y))
    print(f"scale 1e-3: first_order_miss {small.first_order_miss:.3e}, truth {truth_miss(small.dtheta):.3e}, tolerance {tol:.3e}; "
          f"|dlogZ exact - first| {np.max(np.abs(small.dlogZ - small1.dlogZ)):.3e}")
    # O(scale^2) beside O(scale): the remainder is about `scale` of the change itself (0.2 to 2.0 of it at scale 1)
    assert small.first_order_miss <= 1e-2 * small.max_abs_logr
    assert small.first_order_miss <= tol
    assert np.max(np.abs(small.dlogZ - small1.dlogZ)) <= tol and np.max(np.abs(small.means - small1.means)) <= tol
    big = hyper_spread(gpr, X, y, w, n_draws=8, seed=6, laplace=lap, scale=1.0, exact=True)
    big1 = hyper_spread(gpr, X, y, w, n_draws=8, seed=6, laplace=lap, scale=1.0)
    print(f"scale 1: first_order_miss {big.first_order_miss:.3e} of max|log r| {big.max_abs_logr:.3e}; "
          f"|dlogZ exact - first| {np.max(np.abs(big.dlogZ - big1.dlogZ)):.3e}")
    assert np.allclose(big.dtheta, 1e3 * small.dtheta, rtol=1e-12)
    assert big.first_order_miss > 1e3 * tol and np.max(np.abs(big.dlogZ - big1.dlogZ)) > 1e3 * tol
    assert big.first_order_miss > 0.1 * big.max_abs_logr        # the issue's finding: 0.2 to 2.0 of the change at 0.3 in log theta


def test_a_failed_draw_is_dropped_and_counted_and_all_failed_raises(monkeypatch):
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample(80)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.02)
    real = gpr._dev.predict_thetas
    fail = {"rows": [3, 7]}

    def failing(thetas, Xq):
        out = real(thetas, Xq)
        for b in fail["rows"]:
            out["mean"][b], out["lml"][b], out["info"][b] = np.nan, -np.inf, 2
        return out
    monkeypatch.setattr(gpr._dev, "predict_thetas", failing)
    good = [s for s in range(10) if s + 1 not in fail["rows"]]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # no NaN reaches an exp or a log
        r = hyper_spread(gpr, X, y, w, n_draws=10, seed=2, laplace=lap, exact=True)
    assert np.array_equal(np.flatnonzero(r.failed), [2, 6]) and r.failed.sum() == 2
    for name in ("dlogZ", "means", "covs", "ess"):
        arr = getattr(r, name)
        assert len(arr) == 10 and np.isnan(arr[r.failed]).all() and np.isfinite(arr[good]).all(), name
    assert np.all(np.isneginf(r.theta_logw[r.failed])) and np.isfinite(r.theta_logw[good]).all()
    assert np.all(np.isneginf(r.lml[r.failed]))
    monkeypatch.setattr(gpr._dev, "predict_thetas", real)
    whole = hyper_spread(gpr, X, y, w, n_draws=10, seed=2, laplace=lap, exact=True)
    for name in ("dlogZ", "means", "covs", "ess"):      # (8 rows or 10 through the same products: another blocking, rounding apart)
        assert np.allclose(getattr(r, name)[good], getattr(whole, name)[good], rtol=1e-12, atol=1e-15), name
    assert abs(r.logZ_std - whole.dlogZ[good].std()) <= 1e-12 * r.logZ_std and abs(r.ess_min - whole.ess[good].min()) <= 1e-12 * r.ess_min
    assert np.isfinite(r.sigma_theta_draws).all() and np.isfinite(r.first_order_miss) and np.isfinite(r.max_abs_logr)
    assert np.isfinite(r.mean_shift_sigma).all() and np.isfinite(r.cov_ratio_std).all()
    tw = np.exp(r.theta_logw[good])
    assert abs(r.theta_ess - tw.sum() ** 2 / np.sum(tw * tw)) <= 1e-12 * r.theta_ess
    # all fail; and theta itself
    monkeypatch.setattr(gpr._dev, "predict_thetas", failing)
    fail["rows"] = list(range(1, 11))
    with pytest.raises(ValueError, match="not positive definite at any"):
        hyper_spread(gpr, X, y, w, n_draws=10, seed=2, laplace=lap, exact=True)
    fail["rows"] = [0]
    with pytest.raises(ValueError, match="theta itself"):
        hyper_spread(gpr, X, y, w, n_draws=10, seed=2, laplace=lap, exact=True)


def test_theta_logw_is_zero_for_a_gaussian_lml_and_minus_infinity_outside_the_bounds():
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample(40)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.05)
    th0 = np.asarray(lap.theta)
    P = np.linalg.inv(lap.cov)
    # a log marginal likelihood that IS the Laplace Gaussian: the ratio is 1 at every draw
    gpr._dev.lml_fn = lambda th: -7.5 - 0.5 * (th - th0).dot(P).dot(th - th0)
    r = hyper_spread(gpr, X, y, w, n_draws=20, seed=8, laplace=lap, exact=True)
    assert r.lml0 == -7.5 and np.max(np.abs(r.theta_logw)) <= 1e-12 * np.max(np.abs(r.lml - r.lml0))
    assert abs(r.theta_ess - 20.0) <= 1e-9
    # ... at any scale: the draws are from N(0, scale^2 cov), and the ratio is to THAT Gaussian
    gpr._dev.lml_fn = lambda th: -7.5 - 0.5 * (th - th0).dot(P).dot(th - th0) / 0.25
    r = hyper_spread(gpr, X, y, w, n_draws=20, seed=8, laplace=lap, scale=0.5, exact=True)
    assert np.max(np.abs(r.theta_logw)) <= 1e-12 * np.max(np.abs(r.lml - r.lml0))
    # bounds that the draws of the first entry leave upwards: those draws weigh nothing
    gpr._dev.lml_fn = lambda th: -7.5 - 0.5 * (th - th0).dot(P).dot(th - th0)
    bounds = np.array(lap.bounds, dtype=float)
    bounds[0, 1] = th0[0]
    r = hyper_spread(gpr, X, y, w, n_draws=20, seed=8, laplace=lap._replace(bounds=bounds), exact=True)
    out = r.dtheta[:, 0] > 0
    assert out.any() and not out.all()
    assert np.all(np.isneginf(r.theta_logw[out])) and np.max(np.abs(r.theta_logw[~out])) <= 1e-12 * np.max(np.abs(r.lml - r.lml0))
    assert abs(r.theta_ess - float((~out).sum())) <= 1e-9
    assert not r.failed.any() and np.isfinite(r.dlogZ).all()        # (outside the bounds is no failure: the summaries keep the draw)
    # a held entry is not tested against its bounds
    free = np.array([False, True, True, True])
    lap2 = laplace_with(gpr, 0.05, free)._replace(bounds=bounds)
    P2 = np.linalg.inv(lap2.cov)
    gpr._dev.lml_fn = lambda th: -7.5 - 0.5 * (th - th0)[free].dot(P2).dot((th - th0)[free])
    r = hyper_spread(gpr, X, y, w, n_draws=20, seed=8, laplace=lap2, exact=True)
    assert np.all(r.dtheta[:, 0] == 0.0) and np.max(np.abs(r.theta_logw)) <= 1e-12 * np.max(np.abs(r.lml - r.lml0))
