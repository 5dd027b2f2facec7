"""The Hessian of the log marginal likelihood without a GPU: the numpy reference itself (tests/tools/lml_hessian_model.py:
the two formulations against each other and against central differences of the analytic gradient, the zero cross entries
of log w, the r = 0 convention, the not-positive-definite convention) and the host side -- ``gpr.lml_hessian`` and
``hyper_laplace`` -- on the stand-in device.
"""
import copy
import math
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lml_hessian_model as hm  # noqa: E402
from oracle_device import attach  # noqa: E402
from oracle import gpry_oracle as orc  # noqa: E402

from gpry_amd.kernels import RBF, Matern, ConstantKernel as C, WhiteKernel  # noqa: E402


# ------------------------------------------------------------------------------------ the reference
def analytic_gradient(X_, y_, alpha, theta, kid, white):
    """The oracle's gradient; the entry of log w, which the oracle does not carry, is 1/2 w tr(alpha_ alpha_^T - K^-1)."""
    d = X_.shape[1]
    if not white:
        return orc.log_marginal_likelihood(X_, y_, alpha, theta, kid, eval_gradient=True)[1]
    w = math.exp(theta[d + 1])
    g = orc.log_marginal_likelihood(X_, y_, alpha + w, theta[:d + 1], kid, eval_gradient=True)[1]
    K = orc.kernel_matrix(X_, theta[:d + 1], kid)
    K[np.diag_indices_from(K)] += alpha + w
    Kinv = np.linalg.inv(K)
    al = Kinv.dot(y_)
    return np.append(g, 0.5 * w * (al.dot(al) - np.trace(Kinv)))


def central_differences(X_, y_, alpha, theta, kid, white, h=1e-5):
    p = len(theta)
    H = np.empty((p, p))
    for j in range(p):
        e = np.zeros(p)
        e[j] = h
        H[:, j] = (analytic_gradient(X_, y_, alpha, theta + e, kid, white)
                   - analytic_gradient(X_, y_, alpha, theta - e, kid, white)) / (2.0 * h)
    return H


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("N,d", [(40, 1), (90, 3), (150, 8)])
def test_formulations_agree_and_match_central_differences(N, d, kid, white):
    X_, y_, a, theta = hm.problem(N, d, seed=100 * N + d, white=white)
    la, ga, Ha = hm.hessian_explicit(X_, y_, a, theta, kid, white)
    lb, gb, Hb = hm.hessian_via_V(X_, y_, a, theta, kid, white)
    big = np.max(np.abs(Hb))
    fd = central_differences(X_, y_, a, theta, kid, white)
    print(f"lml_hessian n{N}_d{d}_k{kid}{'_w' if white else ''}: a-b {np.max(np.abs(Ha - Hb)) / big:.2e}, differences - b "
          f"{np.max(np.abs(fd - Hb)) / big:.2e} of max|H|")
    assert np.isfinite(Hb).all() and np.array_equal(Hb, Hb.T) and np.array_equal(Ha, Ha.T)       # (row 1 = row 0: r = 0 pairs)
    assert abs(la - lb) <= 1e-10 * (abs(lb) + N)
    assert np.max(np.abs(ga - gb)) <= 1e-9 * np.max(np.abs(gb))
    assert np.max(np.abs(ga - analytic_gradient(X_, y_, a, theta, kid, white))) <= 1e-8 * np.max(np.abs(gb))
    assert np.max(np.abs(Ha - Hb)) <= 1e-9 * big
    assert np.max(np.abs(fd - Hb)) <= 1e-4 * big


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
def test_cross_entries_of_log_w_have_no_second_derivative(kid):
    """K_iw = 0 for every i != w, (log C, log w) included: the entries are the middle term and the pair trace alone."""
    N, d = 60, 3
    X_, y_, a, theta = hm.problem(N, d, seed=11, white=True)
    K, dKs = hm._matrices(X_, a, theta, kid, True)
    Kinv = np.linalg.inv(K)
    al = Kinv.dot(y_)
    w = math.exp(theta[d + 1])
    for f in (hm.hessian_explicit, hm.hessian_via_V):
        _, g, H = f(X_, y_, a, theta, kid, True)
        for i in range(d + 1):
            closed = -w * dKs[i].dot(al).dot(Kinv.dot(al)) + 0.5 * w * np.trace(Kinv.dot(dKs[i]).dot(Kinv))
            assert abs(H[i, d + 1] - closed) <= 1e-9 * np.max(np.abs(H))
        # what writing K_w into (log C, log w) by analogy with the row of log C would add is not small
        assert abs(g[d + 1]) > 1e-6 * np.max(np.abs(H))


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
def test_pairs_at_distance_zero_contribute_nothing(kid):
    X_, y_, a, theta = hm.problem(30, 2, seed=3, white=False)
    Cg, D = hm.second_weight(X_, theta, kid)
    assert np.isfinite(Cg).all() and Cg[0, 1] == 0.0 and Cg[1, 0] == 0.0 and not np.diag(Cg).any()
    assert (Cg[np.triu_indices(30, 2)] > 0).all()
    assert np.isfinite(hm.hessian_via_V(X_, y_, a, theta, kid)[2]).all()


def test_not_positive_definite_convention():
    X_ = np.zeros((6, 2))
    y_ = np.arange(6.0)
    theta = np.log([2.0, 0.3, 0.3])
    for f in (hm.hessian_explicit, hm.hessian_via_V):
        v, g, H = f(X_, y_, np.zeros(6), theta, 0)
        assert v == -np.inf and g.shape == (3,) and not g.any() and H.shape == (3, 3) and not H.any()


# ------------------------------------------------------------------------------------ the regressor on the stand-in
BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0]])
L_BOUNDS = [1e-3, 10.0]


def data(n=36, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


def make_gpr(kernel, X=None, y=None):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    gpr = attach(GaussianProcessRegressor(kernel=kernel, bounds=BOUNDS, n_restarts_optimizer=1, noise_level=1e-2,
                                          preprocessing_X=Normalize_bounds(BOUNDS), preprocessing_y=Normalize_y(),
                                          account_for_inf=None, random_state=3), hm.HessDevice())
    gpr.fit_lockstep = False
    if X is None:
        X, y = data()
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr


def white_kernel(ls=(0.4, 0.7)):
    return C(1.5, [1e-3, 1e4]) * RBF(list(ls), L_BOUNDS) + WhiteKernel(1e-2, [1e-6, 1e1])


def reference(gpr, theta_full, kid, white):
    dev = gpr._dev
    return hm.hessian_via_V(dev.X_, dev.y_, dev.alpha, theta_full, kid, white)


def test_gpr_lml_hessian_is_the_twin_of_the_objective():
    gpr = make_gpr(white_kernel())
    theta = gpr.kernel_.theta.copy()
    n0 = gpr.n_eval_loglike
    lml, g, H = gpr.lml_hessian()
    assert gpr.n_eval_loglike == n0 + 1 and gpr._dev.n_hess == 1
    assert g.shape == (4,) and H.shape == (4, 4) and np.array_equal(H, H.T)
    l2, g2 = gpr.log_marginal_likelihood(theta, eval_gradient=True)
    assert abs(lml - l2) <= 1e-10 * (abs(l2) + 36) and np.max(np.abs(g - g2)) <= 1e-8 * np.max(np.abs(g2))
    lr, gr, Hr = reference(gpr, theta, 0, True)
    assert lml == lr and np.array_equal(H, Hr)
    # at a theta passed in; the kernel keeps its own
    other = theta + 0.1
    assert np.array_equal(gpr.lml_hessian(other)[2], reference(gpr, other, 0, True)[2])
    assert np.array_equal(gpr.kernel_.theta, theta)


def test_gpr_lml_hessian_maps_fixed_isotropic_and_swapped_kernels():
    # no white term, Matern-5/2
    gpr = make_gpr(C(1.5, [1e-3, 1e4]) * Matern([0.4, 0.7], L_BOUNDS, nu=2.5))
    lml, g, H = gpr.lml_hessian()
    assert H.shape == (3, 3) and np.array_equal(H, reference(gpr, gpr.kernel_.theta, 3, False)[2])
    # the white term first: theta = [log w, log C, log l_1, log l_2]
    gpr = make_gpr(WhiteKernel(1e-2, [1e-6, 1e1]) + C(1.5, [1e-3, 1e4]) * RBF([0.4, 0.7], L_BOUNDS))
    th = gpr.kernel_.theta
    full = np.append(th[1:], th[0])
    Hr = reference(gpr, full, 0, True)[2]
    perm = [3, 0, 1, 2]
    assert np.allclose(gpr.lml_hessian()[2], Hr[np.ix_(perm, perm)], rtol=0, atol=1e-12 * np.max(np.abs(Hr)))
    # an isotropic length scale: the second derivative along (1, 1) of the two device entries; a fixed constant drops out
    gpr = make_gpr(C(1.5, "fixed") * RBF(0.5, L_BOUNDS))
    lml, g, H = gpr.lml_hessian()
    full = np.log([1.5, 0.5, 0.5])
    lr, gr, Hr = reference(gpr, full, 0, False)
    assert H.shape == (1, 1) and abs(H[0, 0] - Hr[1:, 1:].sum()) <= 1e-12 * np.max(np.abs(Hr))
    assert abs(g[0] - gr[1:].sum()) <= 1e-12 * np.max(np.abs(gr))


def test_hyper_laplace_report():
    from gpry_amd.mc import hyper_laplace, HyperLaplace
    gpr = make_gpr(white_kernel())
    theta = gpr.kernel_.theta.copy()
    r = hyper_laplace(gpr)
    assert isinstance(r, HyperLaplace)
    lr, gr, Hr = reference(gpr, theta, 0, True)
    assert r.names == ["log C", "log l_1", "log l_2", "log w"]
    assert np.array_equal(r.theta, theta) and r.lml == lr and np.array_equal(r.grad, gr) and np.array_equal(r.H, Hr)
    assert np.allclose(r.bounds, np.log([[1e-3, 1e4], L_BOUNDS, L_BOUNDS, [1e-6, 1e1]]))
    assert r.free.all() and r.free.dtype == bool
    A = -Hr
    try:
        L = np.linalg.cholesky(A)
        negdef = True
    except np.linalg.LinAlgError:
        negdef = False
    assert r.negdef == negdef
    w, v = np.linalg.eigh(A)
    assert np.allclose(r.eigvals, w) and (np.diff(r.eigvals) >= 0).all() and r.eigvecs.shape == (4, 4)
    if negdef:
        assert np.max(np.abs(r.cov.dot(A) - np.eye(4))) <= 1e-8
        assert np.allclose(r.sigma_log, np.sqrt(np.diag(r.cov))) and np.allclose(np.diag(r.corr), 1.0)
        ev = lr + 2.0 * math.log(2.0 * math.pi) - np.sum(np.log(np.diag(L))) - np.sum(np.log(r.bounds[:, 1] - r.bounds[:, 0]))
        assert abs(r.log_evidence - ev) <= 1e-10 * abs(ev)
    else:
        assert r.cov is None and r.corr is None and np.isnan(r.sigma_log).all() and math.isnan(r.log_evidence)
    assert r.device_s == 0.0 and r.wall_s > 0.0
    # at a theta passed in
    assert np.array_equal(hyper_laplace(gpr, theta - 0.2).H, reference(gpr, theta - 0.2, 0, True)[2])


def test_hyper_laplace_after_a_fit_finds_a_maximum_over_the_free_entries():
    from gpry_amd.mc import hyper_laplace
    gpr = make_gpr(white_kernel())
    gpr.fit_gpr_hyperparameters()
    r = hyper_laplace(gpr)
    A = -r.H[np.ix_(r.free, r.free)]
    # L-BFGS-B ends at a maximum over the entries that are not held by a bound: there the curvature is negative
    assert r.free.any() and r.negdef
    assert np.max(np.abs(r.grad[r.free])) <= 1e-3 * np.max(np.abs(r.H))
    assert np.max(np.abs(r.cov.dot(A) - np.eye(len(A)))) <= 1e-8
    assert (r.eigvals > 0).all() and np.isfinite(r.sigma_log[r.free]).all() and np.isnan(r.sigma_log[~r.free]).all()
    assert math.isnan(r.log_evidence) == (not r.free.all())


def test_hyper_laplace_holds_entries_on_a_bound_and_fixed_ones():
    from gpry_amd.mc import hyper_laplace
    # y does not depend on the second coordinate: at the upper bound of l_2 the likelihood still rises
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (40, 2))
    y = np.sin(5 * X[:, 0]) + 0.05 * rng.standard_normal(40)
    gpr = make_gpr(white_kernel(ls=(0.4, L_BOUNDS[1])), X, y)
    r = hyper_laplace(gpr)
    assert r.theta[2] == math.log(L_BOUNDS[1]) and r.grad[2] > 0
    assert list(r.free) == [True, True, False, True]
    assert math.isnan(r.log_evidence) and math.isnan(r.sigma_log[2])
    f = r.free
    if r.negdef:
        assert r.cov.shape == (3, 3) and np.max(np.abs(r.cov.dot(-r.H[np.ix_(f, f)]) - np.eye(3))) <= 1e-8
        assert np.isfinite(r.sigma_log[f]).all()
    # the same entry on the bound with the gradient pointing inward stays free
    gpr = make_gpr(white_kernel(ls=(0.4, L_BOUNDS[0])), X, y)
    r = hyper_laplace(gpr)
    assert r.theta[2] == math.log(L_BOUNDS[0])
    assert bool(r.free[2]) == bool(r.grad[2] > 0)
    # a fixed constant is held, its bounds are its value
    gpr = make_gpr(C(1.5, "fixed") * RBF([0.4, 0.7], L_BOUNDS), X, y)
    r = hyper_laplace(gpr)
    assert r.names == ["log C", "log l_1", "log l_2"] and not r.free[0] and r.bounds[0, 0] == r.bounds[0, 1] == r.theta[0]
    assert math.isnan(r.log_evidence) and math.isnan(r.sigma_log[0])
    # an isotropic length scale ties two entries of the device's vector
    with pytest.raises(ValueError, match="isotropic"):
        hyper_laplace(make_gpr(C(1.5, [1e-3, 1e4]) * RBF(0.5, L_BOUNDS), X, y))


def test_not_positive_definite_model_reports_nothing():
    from gpry_amd.mc import hyper_laplace
    gpr = make_gpr(C(2.0, [1e-3, 1e4]) * RBF([0.3, 0.3], L_BOUNDS))
    dev = gpr._dev
    gpr.lml_hessian()       # (uploads the training set)
    dev.set_train(np.zeros((6, 2)), np.arange(6.0), np.zeros(6))
    gpr.y_train_ = np.arange(6.0)
    lml, g, H = gpr.lml_hessian()
    assert lml == -np.inf and not g.any() and not H.any() and H.shape == (3, 3)
    r = hyper_laplace(gpr)
    assert r.lml == -np.inf and not r.negdef and r.cov is None and math.isnan(r.log_evidence) and np.isnan(r.sigma_log).all()


def test_result_survives_copy_and_pickle_of_the_regressor():
    from gpry_amd.mc import hyper_laplace
    gpr = make_gpr(white_kernel())
    r = hyper_laplace(gpr)
    for c in (copy.deepcopy(gpr), pickle.loads(pickle.dumps(gpr))):
        attach(c, hm.HessDevice())
        c._dev_train_ok = False
        rc = hyper_laplace(c)
        assert np.array_equal(rc.H, r.H) and rc.lml == r.lml and np.array_equal(rc.free, r.free)
        assert np.array_equal(rc.log_evidence, r.log_evidence, equal_nan=True)
    # the result itself is plain data
    back = pickle.loads(pickle.dumps(r))
    assert np.array_equal(back.H, r.H) and back.names == r.names
    assert np.array_equal(copy.deepcopy(r).free, r.free)
