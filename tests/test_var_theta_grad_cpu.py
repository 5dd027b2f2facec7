"""The derivative of the predictive variance in theta without a GPU: the numpy reference itself (tests/tools/
var_theta_grad_model.py: two closed-form formulations against each other and against central differences of the refactorised
variance), the shared assertions on the stand-in device -- and on three broken stand-ins, which they must catch -- and the
host side: ``gpr.var_theta_grad`` and ``hyper_acq_spread`` against a direct evaluation of its formulas.
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import var_theta_grad_model as vm  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd.kernels import RBF, Matern, ConstantKernel as C, WhiteKernel  # noqa: E402

SMALL = [(50, 1, 1, False), (130, 2, 3, True), (333, 5, 2, True)]


# ------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("N,d", [(50, 1), (130, 2), (333, 5)])
def test_the_two_formulations_agree_and_match_central_differences(N, d, kid, white):
    """(a) against (b) per column over the 26 points of the device tests: 1e-8 of the column's largest entry (seen: 1e-13 to
    1.5e-9, cond(K) ~ 1e6 times the rounding of q).  Central differences, without the two far points, with h = 1e-4: the
    truncation is h^2 / 6 of the third derivative (2e-9 times a few tens), the rounding of the variance (cond(K) times 1e-16 of C) divided by 2 h a few 1e-7 of the largest entry: 2e-5 of
    the largest entry of G is the bound, as for the mean's derivative."""
    case = (N, d, kid, white)
    X_, y_, a, th = vm.problem(N, d, seed=N + d, white=white)
    Xq_ = vm.points(case, X_)
    va, Ga = vm.grad_explicit(X_, a, th, kid, white, Xq_, vm.Y_STD)
    vb, Gb = vm.grad_via_V(X_, a, th, kid, white, Xq_, vm.Y_STD)
    fd = vm.central_differences(X_, a, th, kid, white, Xq_[:24], vm.Y_STD, h=1e-4)
    colmax, big = np.max(np.abs(Gb), axis=0), np.max(np.abs(Gb[:24]))
    print(f"n{N}_d{d}_k{kid}{'_w' if white else ''}: a - b {np.max(np.max(np.abs(Ga - Gb), axis=0) / colmax):.2e} of the column, "
          f"closed form - differences {np.max(np.abs(fd - Gb[:24])) / big:.2e} of the largest entry")
    assert np.all(np.max(np.abs(Ga - Gb), axis=0) <= 1e-8 * colmax)
    assert np.max(np.abs(fd - Gb[:24])) <= 2e-5 * big
    assert np.array_equal(Gb[-2:], np.tile(vm.far_rows(case, th), (2, 1))) and np.array_equal(Ga[-2:], Gb[-2:])
    ref = vm.var_numpy(X_, a, th, kid, white, Xq_, vm.Y_STD)
    assert np.max(np.abs(va - ref)) <= 1e-8 * np.max(ref) and np.max(np.abs(vb - ref)) <= 1e-8 * np.max(ref)


# ------------------------------------------------------------------------------------ the assertions on the stand-in
@pytest.mark.parametrize("case", SMALL)
def test_stand_in_passes_every_check(case):
    dev, other = vm.VarThetaGradDevice(), vm.VarThetaGradDevice()
    vm.check_closed_form(dev, case)
    vm.check_var(dev, case)
    vm.check_same_bits(dev, case, other)


def test_stand_in_passes_the_check_against_its_own_differences():
    vm.check_against_own_differences(vm.VarThetaGradDevice(), (130, 2, 1, True))


BROKEN = [("quad_sign", -1.0), ("cross_factor", 1.0), ("logc_noise", False)]


@pytest.mark.parametrize("name,value", BROKEN)
@pytest.mark.parametrize("case", SMALL)
def test_a_broken_variant_fails_the_closed_form_check(case, name, value):
    """The sign of the quadratic term, a missing factor 2 on the cross term, the log C column without the noise term."""
    dev = vm.VarThetaGradDevice()
    setattr(dev, name, value)
    with pytest.raises(AssertionError):
        vm.check_closed_form(dev, case)


@pytest.mark.parametrize("name,value", BROKEN)
def test_the_check_against_the_device_s_own_differences_catches_them_too(name, value):
    dev = vm.VarThetaGradDevice()
    setattr(dev, name, value)
    with pytest.raises(AssertionError):
        vm.check_against_own_differences(dev, (130, 2, 0, False))


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
                                          account_for_inf=None, random_state=3), vm.VarThetaGradDevice())
    gpr.fit_lockstep = False
    gpr.append_to_data(*data(), fit_gpr=False)
    return gpr


def white_kernel(ls=(0.4, 0.7)):
    return C(1.5, [1e-3, 1e4]) * RBF(list(ls), L_BOUNDS) + WhiteKernel(1e-2, [1e-6, 1e1])


def sample(n, seed=9):
    return np.random.default_rng(seed).uniform(0, 1, (n, 2))


def reference(gpr, X, theta_full, kid, white):
    dev = gpr._dev
    return vm.grad_via_V(dev.X_, dev.alpha, theta_full, kid, white, dev._to_unit(X), dev.y_std)


def test_gpr_var_theta_grad_full_and_mapped_and_its_refusals():
    X = sample(30)
    gpr = make_gpr(white_kernel())
    n0 = gpr.n_eval
    var, G = gpr.var_theta_grad(X, full=True)
    assert gpr.n_eval == n0 + 30 and gpr._dev.n_vtg == 1 and G.shape == (30, 4) and var.shape == (30,)
    vr, Gr = reference(gpr, X, gpr.kernel_.theta, 0, True)
    assert np.allclose(G, Gr, rtol=0, atol=1e-12 * np.max(np.abs(Gr))) and np.allclose(var, vr, rtol=0, atol=1e-12 * np.max(vr))
    assert np.array_equal(gpr.var_theta_grad(X)[1], G)              # theta is the device's own vector
    # the white term first: theta = [log w, log C, log l_1, log l_2]
    gpr = make_gpr(WhiteKernel(1e-2, [1e-6, 1e1]) + C(1.5, [1e-3, 1e4]) * RBF([0.4, 0.7], L_BOUNDS))
    th = gpr.kernel_.theta
    G = gpr.var_theta_grad(X)[1]                        # (the call pushes the affine maps the reference reads)
    _, Gr = reference(gpr, X, np.append(th[1:], th[0]), 0, True)
    assert np.allclose(G, Gr[:, [3, 0, 1, 2]], rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    assert np.allclose(gpr.var_theta_grad(X, full=True)[1], Gr, rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    # an isotropic length scale sums its tied columns; a fixed constant drops out
    gpr = make_gpr(C(1.5, "fixed") * Matern(0.5, L_BOUNDS, nu=2.5))
    _, G = gpr.var_theta_grad(X)
    _, Gr = reference(gpr, X, np.log([1.5, 0.5, 0.5]), 3, False)
    assert G.shape == (30, 1) and np.allclose(G[:, 0], Gr[:, 1:].sum(axis=1), rtol=0, atol=1e-12 * np.max(np.abs(Gr)))
    assert gpr.var_theta_grad(X, full=True)[1].shape == (30, 3)
    # the refusals: a coordinate that is not finite, a wrong width, no rows, no data
    with pytest.raises(ValueError):
        gpr.var_theta_grad(np.array([[0.1, np.nan]]))
    with pytest.raises(ValueError, match="dimension 2"):
        gpr.var_theta_grad(np.zeros((3, 5)))
    with pytest.raises(ValueError, match="dimension 2"):
        gpr.var_theta_grad(np.zeros((0, 2)))
    from gpry_amd.gpr import GaussianProcessRegressor
    empty = attach(GaussianProcessRegressor(kernel=white_kernel(), bounds=BOUNDS, account_for_inf=None), vm.VarThetaGradDevice())
    with pytest.raises(ValueError, match="training data"):
        empty.var_theta_grad(X, validate=False)


def laplace_with(gpr, cov_diag, free=None):
    """The report of the model with a covariance put in by hand (the stand-in's model is not at an optimum)."""
    from gpry_amd.mc import hyper_laplace
    lap = hyper_laplace(gpr)
    p = len(lap.theta)
    free = np.ones(p, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    k = int(free.sum())
    A = np.random.default_rng(2).standard_normal((k, k)) * 0.2 + np.eye(k)
    return lap._replace(negdef=True, free=free, cov=cov_diag * A.dot(A.T))


def phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def direct(gpr, X, lap, zeta, sigma_n, scale):
    """``hyper_acq_spread``'s formulas written out row by row from the two calls."""
    mean, Gm = gpr.mean_theta_grad(X, full=True)
    var, Gv = gpr.var_theta_grad(X, full=True)
    S = scale ** 2 * np.asarray(lap.cov)
    f = np.flatnonzero(lap.free)
    n = len(X)
    acq, grad, srel, asig = np.full(n, -np.inf), np.full((n, Gm.shape[1]), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        if var[i] > 0:
            srel[i] = math.sqrt(Gv[i, f].dot(S).dot(Gv[i, f])) / (2.0 * var[i])
        if var[i] - sigma_n ** 2 > 0 and np.isfinite(mean[i]):
            acq[i] = 2.0 * zeta * (mean[i] - gpr.y_max) + 0.5 * math.log(var[i] - sigma_n ** 2)
            grad[i] = 2.0 * zeta * Gm[i] + Gv[i] / (2.0 * (var[i] - sigma_n ** 2))
            asig[i] = math.sqrt(grad[i, f].dot(S).dot(grad[i, f]))
    flip = np.full((n, n), np.nan)
    for i in range(n):
        for j in range(n):
            if np.isfinite(acq[i]) and np.isfinite(acq[j]):
                dg = grad[i, f] - grad[j, f]
                s = math.sqrt(max(dg.dot(S).dot(dg), 0.0))
                gap = abs(acq[i] - acq[j])
                flip[i, j] = phi(-gap / s) if s > 0 else (0.5 if gap == 0 else 0.0)
    return mean, var, acq, grad, srel, asig, flip


def test_hyper_acq_spread_equals_the_direct_evaluation_of_its_formulas():
    from gpry_amd.acquisition_functions import LogExp
    from gpry_amd.mc import HyperAcqSpread, hyper_acq_spread
    gpr = make_gpr(white_kernel())
    X = np.vstack([sample(20), gpr.X_train[:6]])          # the training rows: var of the order of the noise
    lap = laplace_with(gpr, 0.02, free=[True, True, False, True])
    var0 = gpr.var_theta_grad(X, full=True)[0]
    sigma_n = float(np.sqrt(np.sort(var0)[3:5].mean()))   # four rows with var <= sigma_n^2
    acq = LogExp(zeta=0.3, sigma_n=sigma_n)
    n0, c0 = gpr.n_eval, (gpr._dev.n_tg, gpr._dev.n_vtg)
    r = hyper_acq_spread(gpr, X, acq=acq, laplace=lap, scale=1.5)
    assert isinstance(r, HyperAcqSpread) and gpr.n_eval == n0 + 2 * len(X)
    assert (gpr._dev.n_tg, gpr._dev.n_vtg) == (c0[0] + 1, c0[1] + 1)        # one call each
    mean, var, a, grad, srel, asig, flip = direct(gpr, X, lap, 0.3, sigma_n, 1.5)
    dead = ~np.isfinite(a)
    assert dead.sum() == 4 and np.array_equal(np.isneginf(r.acq), dead) and np.all(np.isnan(r.acq_grad[dead]))
    assert np.array_equal(r.mean, mean) and np.array_equal(r.var, var) and r.zeta == 0.3 and r.sigma_n == sigma_n
    assert r.baseline == gpr.y_max and r.device_ms == 0.0
    assert np.allclose(r.sigma, np.sqrt(var), rtol=1e-15) and np.allclose(r.sigma_rel_theta, srel, rtol=1e-12, equal_nan=True)
    assert np.allclose(r.acq[~dead], a[~dead], rtol=0, atol=1e-13) and np.allclose(r.acq_grad, grad, rtol=1e-13, equal_nan=True)
    assert np.allclose(r.acq_sigma_theta, asig, rtol=1e-12, equal_nan=True)
    assert np.array_equal(r.order, np.argsort(-a, kind="stable")) and np.all(np.diff(r.acq[r.order][:len(X) - 4]) <= 0)
    assert np.allclose(r.flip, flip, rtol=1e-10, atol=1e-300, equal_nan=True)
    live = np.flatnonzero(~dead)
    assert np.allclose(r.flip[np.ix_(live, live)], r.flip[np.ix_(live, live)].T) and np.all(np.diag(r.flip)[live] == 0.5)
    top = r.order[0]
    want = flip[:, top].copy()
    want[top] = 0.0
    assert np.allclose(r.top_flip, want, rtol=1e-10, atol=1e-300, equal_nan=True) and np.all(np.isnan(r.top_flip[dead]))
    # held entries carry no spread: the column of log l_2 does not enter
    Gv = r.G_var.copy()
    assert np.allclose(r.sigma_rel_theta[~dead],
                       (1.5 * np.sqrt(np.einsum("if,fg,ig->i", Gv[:, lap.free], lap.cov, Gv[:, lap.free])) / (2 * var))[~dead],
                       rtol=1e-12)
    # None: LogExp(dimension = d), its sigma_n from the regressor's noise level
    r2 = hyper_acq_spread(gpr, X, laplace=lap)
    assert r2.zeta == LogExp(dimension=2).zeta and r2.sigma_n == LogExp(dimension=2)._noise(gpr)[0] and r2.scale == 1.0


def test_hyper_acq_spread_above_256_rows_gives_no_table_and_refuses_without_a_covariance():
    from gpry_amd.mc import hyper_acq_spread
    gpr = make_gpr(white_kernel())
    lap = laplace_with(gpr, 0.02)
    X = sample(257)
    r = hyper_acq_spread(gpr, X, laplace=lap)
    assert r.flip is None and r.top_flip.shape == (257,) and r.order.shape == (257,) and r.top_flip[r.order[0]] == 0.0
    few = hyper_acq_spread(gpr, X[:256], laplace=lap)
    assert few.flip.shape == (256, 256)
    # a row's figures do not depend on the rows beside it; top_flip against the same top row is the table's column
    assert np.array_equal(few.acq, r.acq[:256]) and np.array_equal(few.acq_sigma_theta, r.acq_sigma_theta[:256])
    assert np.allclose(few.top_flip, np.where(np.arange(256) == few.order[0], 0.0, few.flip[:, few.order[0]]), rtol=1e-12)
    with pytest.raises(ValueError, match="negdef"):
        hyper_acq_spread(gpr, X, laplace=lap._replace(negdef=False, cov=None))
    with pytest.raises(ValueError, match="free"):
        hyper_acq_spread(gpr, X, laplace=lap._replace(free=np.zeros(4, dtype=bool), cov=np.zeros((0, 0))))
    with pytest.raises(ValueError, match="scale"):
        hyper_acq_spread(gpr, X, laplace=lap, scale=0.0)
