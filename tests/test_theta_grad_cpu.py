"""The derivative of the posterior mean in theta without a GPU: the numpy reference itself (tests/tools/theta_grad_model.py:
the closed form against central differences of the numpy mean), the shared assertions on the stand-in device -- and on two
broken stand-ins, which they must catch -- and the host side: ``gpr.mean_theta_grad`` and ``hyper_spread``.
"""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import theta_grad_model as tm  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd.kernels import RBF, Matern, ConstantKernel as C, WhiteKernel  # noqa: E402

SMALL = [(50, 1, 1, False), (130, 2, 3, True), (333, 5, 2, True)]


# ------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("N,d", [(50, 1), (130, 2), (333, 5)])
def test_closed_form_matches_central_differences(N, d, kid, white):
    """h = 1e-4: the truncation is h^2 / 6 of the third derivative (2e-9 times a few tens), the rounding of the mean
    (cond(K) ~ 1e6 times 1e-16 of its size) divided by 2 h is a few 1e-7 of the largest entry: 2e-5 of it is the bound.
    Of the largest entry of G, not per column: the log C column is 1e-3 of the others and carries the same absolute
    noise of the differences."""
    case = (N, d, kid, white)
    X_, y_, a, th = tm.problem(N, d, seed=N + d, white=white)
    Xq_ = tm.points(case, X_)[:24]
    Ga = tm.grad_explicit(X_, y_, a, th, kid, white, Xq_, tm.Y_STD)
    Gb = tm.grad_via_V(X_, y_, a, th, kid, white, Xq_, tm.Y_STD)
    fd = tm.central_differences(X_, y_, a, th, kid, white, Xq_, tm.Y_STD, h=1e-4)
    big = np.max(np.abs(Gb))
    print(f"n{N}_d{d}_k{kid}{'_w' if white else ''}: closed form - differences {np.max(np.abs(fd - Gb)) / big:.2e}, "
          f"a - b {np.max(np.abs(Ga - Gb)) / big:.2e} of the largest entry")
    assert np.max(np.abs(Ga - Gb)) <= 1e-8 * big
    assert np.max(np.abs(fd - Gb)) <= 2e-5 * big


# ------------------------------------------------------------------------------------ the assertions on the stand-in
@pytest.mark.parametrize("case", SMALL)
def test_stand_in_passes_every_check(case):
    dev, other = tm.ThetaGradDevice(), tm.ThetaGradDevice()
    tm.check_closed_form(dev, case)
    tm.check_value_clip_gates(dev, case)
    tm.check_same_bits(dev, case, other)


def test_stand_in_passes_the_check_against_its_own_differences():
    tm.check_against_own_differences(tm.ThetaGradDevice(), (130, 2, 1, True))


@pytest.mark.parametrize("case", SMALL)
def test_a_wrong_sign_of_the_log_c_column_is_caught(case):
    dev = tm.ThetaGradDevice()
    dev.logc_sign = -1.0
    with pytest.raises(AssertionError):
        tm.check_closed_form(dev, case)


@pytest.mark.parametrize("case", SMALL)
def test_length_scale_columns_off_by_1e_5_are_caught(case):
    dev = tm.ThetaGradDevice()
    dev.ls_factor = 1.0 + 1e-5
    with pytest.raises(AssertionError):
        tm.check_closed_form(dev, case)


def test_the_check_against_the_device_s_own_differences_catches_them_too():
    dev = tm.ThetaGradDevice()
    dev.ls_factor = 1.0 + 1e-5
    with pytest.raises(AssertionError):
        tm.check_against_own_differences(dev, (130, 2, 0, False))


# ------------------------------------------------------------------------------------ the regressor on the stand-in
BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0]])
L_BOUNDS = [1e-3, 10.0]


def data(n=36, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


def make_gpr(kernel):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    gpr = attach(GaussianProcessRegressor(kernel=kernel, bounds=BOUNDS, n_restarts_optimizer=1, noise_level=1e-2,
                                          preprocessing_X=Normalize_bounds(BOUNDS), preprocessing_y=Normalize_y(),
                                          account_for_inf=None, random_state=3), tm.ThetaGradDevice())
    gpr.fit_lockstep = False
    gpr.append_to_data(*data(), fit_gpr=False)
    return gpr


def white_kernel(ls=(0.4, 0.7)):
    return C(1.5, [1e-3, 1e4]) * RBF(list(ls), L_BOUNDS) + WhiteKernel(1e-2, [1e-6, 1e1])


def sample(n=200, seed=9):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (n, 2)), rng.uniform(0.5, 1.5, n)


def reference_G(gpr, X, theta_full, kid, white):
    dev = gpr._dev
    return tm.grad_via_V(dev.X_, dev.y_, dev.alpha, theta_full, kid, white, dev._to_unit(X), dev.y_std)


def test_gpr_mean_theta_grad_full_and_mapped():
    X, _ = sample(30)
    gpr = make_gpr(white_kernel())
    n0 = gpr.n_eval
    mean, G = gpr.mean_theta_grad(X, full=True)
    assert gpr.n_eval == n0 + 30 and gpr._dev.n_tg == 1 and G.shape == (30, 4)
    assert np.allclose(mean, gpr.predict(X), rtol=0, atol=1e-12)
    Gr = reference_G(gpr, X, gpr.kernel_.theta, 0, True)
    assert np.allclose(G, Gr, rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    assert np.array_equal(gpr.mean_theta_grad(X)[1], G)             # theta is the device's own vector
    # the white term first: theta = [log w, log C, log l_1, log l_2]
    gpr = make_gpr(WhiteKernel(1e-2, [1e-6, 1e1]) + C(1.5, [1e-3, 1e4]) * RBF([0.4, 0.7], L_BOUNDS))
    th = gpr.kernel_.theta
    G = gpr.mean_theta_grad(X)[1]                       # (the call pushes the affine maps the reference reads)
    Gr = reference_G(gpr, X, np.append(th[1:], th[0]), 0, True)
    assert np.allclose(G, Gr[:, [3, 0, 1, 2]], rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    assert np.allclose(gpr.mean_theta_grad(X, full=True)[1], Gr, rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    # an isotropic length scale sums its tied columns; a fixed constant drops out
    gpr = make_gpr(C(1.5, "fixed") * Matern(0.5, L_BOUNDS, nu=2.5))
    _, G = gpr.mean_theta_grad(X)
    Gr = reference_G(gpr, X, np.log([1.5, 0.5, 0.5]), 3, False)
    assert G.shape == (30, 1) and np.allclose(G[:, 0], Gr[:, 1:].sum(axis=1), rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    assert gpr.mean_theta_grad(X, full=True)[1].shape == (30, 3)
    with pytest.raises(ValueError):
        gpr.mean_theta_grad(np.array([[0.1, np.nan]]))
    with pytest.raises(ValueError):
        gpr.mean_theta_grad(np.zeros((3, 5)))


def laplace_with(gpr, cov_diag, free=None):
    """The report of the model with a covariance put in by hand (the stand-in's model is not at an optimum)."""
    from gpry_amd.mc import hyper_laplace
    lap = hyper_laplace(gpr)
    p = len(lap.theta)
    free = np.ones(p, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    k = int(free.sum())
    rng = np.random.default_rng(2)
    A = rng.standard_normal((k, k)) * 0.2 + np.eye(k)
    cov = cov_diag * A.dot(A.T)
    return lap._replace(negdef=True, free=free, cov=cov)


def direct(r, X, w, G):
    """surrogate_spread's summaries from the returned draws and G, written out."""
    keep = r.keep
    wk = w[keep] / w[keep].sum()
    logr = r.dtheta.dot(G[keep].T)
    a = np.log(wk)[None, :] + logr
    top = a.max(axis=1)
    e = np.exp(a - top[:, None])
    tot = e.sum(axis=1)
    ws = e / tot[:, None]
    means = ws.dot(X[keep])
    cen = X[keep][None, :, :] - means[:, None, :]
    return top + np.log(tot), means, np.einsum("si,sia,sib->sab", ws, cen, cen), 1.0 / np.sum(ws * ws, axis=1), logr


def test_hyper_spread_equals_the_direct_evaluation_and_is_reproducible():
    from gpry_amd.mc import hyper_spread, HyperSpread
    gpr = make_gpr(white_kernel())
    X, w = sample()
    w[:5] = 0.0
    y = gpr.predict(X)
    y[5:8] = -np.inf
    lap = laplace_with(gpr, 0.02)
    r = hyper_spread(gpr, X, y, w, n_draws=32, seed=4, laplace=lap, scale=1.5)
    assert isinstance(r, HyperSpread) and r.n_points == 192 and np.array_equal(r.keep, np.arange(8, 200)) and r.seed == 4
    again = hyper_spread(gpr, X, y, w, n_draws=32, seed=4, laplace=lap, scale=1.5)
    for name in ("dtheta", "dlogZ", "means", "covs", "ess", "sigma_theta"):
        assert np.array_equal(getattr(r, name), getattr(again, name)), name
    assert not np.array_equal(hyper_spread(gpr, X, y, w, n_draws=32, seed=5, laplace=lap).dtheta, r.dtheta)
    # the draws: through the Cholesky factor of cov from default_rng(seed)
    z = np.random.default_rng(4).standard_normal((32, 4))
    assert np.allclose(r.dtheta, 1.5 * z.dot(np.linalg.cholesky(lap.cov).T), rtol=0, atol=1e-15)
    G = gpr.mean_theta_grad(X, full=True)[1]
    dlogZ, means, covs, ess, logr = direct(r, X, w, G)
    assert np.allclose(r.dlogZ, dlogZ, rtol=0, atol=1e-12) and np.allclose(r.means, means, rtol=0, atol=1e-13)
    assert np.allclose(r.covs, covs, rtol=0, atol=1e-13) and np.allclose(r.ess, ess, rtol=1e-12)
    assert np.allclose(r.mean0, (w[r.keep] / w[r.keep].sum()).dot(X[r.keep]), rtol=0, atol=1e-14)
    assert abs(r.logZ_std - dlogZ.std()) <= 1e-12 and r.ess_min == r.ess.min()
    assert abs(r.max_abs_logr - np.max(np.abs(logr))) <= 1e-12
    var0 = np.diag(r.cov0)
    assert np.allclose(r.mean_shift_sigma, means.std(axis=0) / np.sqrt(var0), rtol=1e-9)
    assert np.allclose(r.cov_ratio_std, (np.einsum("saa->sa", covs) / var0).std(axis=0), rtol=1e-9)
    assert np.allclose(r.sigma_theta, 1.5 * np.sqrt(np.einsum("if,fg,ig->i", G[r.keep], lap.cov, G[r.keep])), rtol=1e-12)
    # None: the report is made here -- and says that this theta is no maximum, or gives a covariance
    from gpry_amd.mc import hyper_laplace
    if hyper_laplace(gpr).negdef and hyper_laplace(gpr).free.any():
        assert hyper_spread(gpr, X, y, w, n_draws=4, seed=1).n_points == 192
    else:
        with pytest.raises(ValueError):
            hyper_spread(gpr, X, y, w, n_draws=4, seed=1)


def test_hyper_spread_holds_the_entries_that_are_not_free_and_refuses_without_a_covariance():
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample(80)
    y = gpr.predict(X)
    free = np.array([True, False, True, False])
    lap = laplace_with(gpr, 0.02, free)
    r = hyper_spread(gpr, X, y, w, n_draws=16, seed=2, laplace=lap)
    assert np.all(r.dtheta[:, ~free] == 0.0) and np.all(r.dtheta[:, free] != 0.0)
    G = gpr.mean_theta_grad(X, full=True)[1]
    assert np.allclose(r.sigma_theta, np.sqrt(np.einsum("if,fg,ig->i", G[:, free], lap.cov, G[:, free])), rtol=1e-12)
    with pytest.raises(ValueError, match="negdef"):
        hyper_spread(gpr, X, y, w, laplace=lap._replace(negdef=False, cov=None))
    with pytest.raises(ValueError, match="free"):
        hyper_spread(gpr, X, y, w, laplace=lap._replace(free=np.zeros(4, dtype=bool), cov=np.zeros((0, 0))))
    with pytest.raises(ValueError):
        hyper_spread(gpr, X, y, w, n_draws=1, laplace=lap)
    with pytest.raises(ValueError):
        hyper_spread(gpr, X, y, np.zeros(80), laplace=lap)


def test_a_constant_column_moves_log_z_alone(monkeypatch):
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample(120)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.05)
    c, j = 0.37, 2
    real = gpr._dev.mean_theta_grad

    def constant(Xq):
        out = real(Xq)
        out["G"] = np.zeros_like(out["G"])
        out["G"][:, j] = c
        return out
    monkeypatch.setattr(gpr._dev, "mean_theta_grad", constant)
    r = hyper_spread(gpr, X, y, w, n_draws=24, seed=8, laplace=lap)
    assert np.allclose(r.dlogZ, c * r.dtheta[:, j], rtol=0, atol=1e-14)
    assert np.allclose(r.means, r.mean0[None, :], rtol=0, atol=1e-14) and np.allclose(r.covs, r.cov0[None], rtol=0, atol=1e-14)
    assert np.allclose(r.ess, 1.0 / np.sum((w / w.sum()) ** 2), rtol=1e-12)


def test_low_effective_sample_size_warns_in_the_words_of_its_twin():
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(white_kernel())
    X, w = sample(300)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.02)
    with pytest.warns(UserWarning, match=r"smallest effective sample size over the draws is .* of 300 rows \(< 5 %\)"):
        r = hyper_spread(gpr, X, y, w, n_draws=8, seed=3, laplace=lap, scale=400.0)
    assert r.ess_min < 15 and r.max_abs_logr > 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hyper_spread(gpr, X, y, w, n_draws=8, seed=3, laplace=lap, scale=0.1)


@pytest.mark.parametrize("kernel,kid,white", [(white_kernel(), 0, True),
                                              (C(1.5, [1e-3, 1e4]) * Matern([0.4, 0.7], L_BOUNDS, nu=1.5), 2, False)])
def test_the_remainder_of_the_linearisation_is_quadratic(kernel, kid, white):
    """Exact log r from refactorising the numpy model at theta + dtheta_s; its distance to the linear one at scale s / 2 is at
    most 0.35 of that at scale s (quadratic remainder: 0.25; the margin is for the cubic term)."""
    from gpry_amd.mc import hyper_spread
    gpr = make_gpr(kernel)
    dev = gpr._dev
    X, w = sample(60)
    y = gpr.predict(X)
    lap = laplace_with(gpr, 0.03 ** 2)
    G = gpr.mean_theta_grad(X, full=True)[1]
    th = np.asarray(lap.theta, dtype=float)

    def exact(dth):
        f = [tm.mean_numpy(dev.X_, dev.y_, dev.alpha, th + s * dth, kid, white, dev._to_unit(X), dev.y_mean, dev.y_std)
             for s in (1.0, 0.0)]
        return f[0] - f[1]
    s = 1.0
    full = hyper_spread(gpr, X, y, w, n_draws=4, seed=6, laplace=lap, scale=s)
    half = hyper_spread(gpr, X, y, w, n_draws=4, seed=6, laplace=lap, scale=s / 2)
    assert np.allclose(half.dtheta, 0.5 * full.dtheta, rtol=0, atol=1e-16)
    checked = 0
    for k in range(4):
        err_s = np.max(np.abs(exact(full.dtheta[k]) - G.dot(full.dtheta[k])))
        err_h = np.max(np.abs(exact(half.dtheta[k]) - G.dot(half.dtheta[k])))
        print(f"draw {k}: remainder {err_s:.3e} at s, {err_h:.3e} at s / 2, ratio {err_h / err_s:.3f}")
        if err_s < 1e-9:
            continue
        checked += 1
        assert err_h <= 0.35 * err_s
    assert checked >= 1
