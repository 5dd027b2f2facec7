"""``gpry_loo_objective`` on the device: the leave-one-out log predictive density of the training targets and its
theta-gradient against the numpy closed form (tests/tools/loo_fit_model.py, formulation (b); the allowed deviation is ten
times the disagreement of the two numpy formulations on the same model, but not below the bounds of the LML on the same
chain, test_white_noise_gpu.py: 1e-10 (|ref| + N) for the value, 1e-7 of the largest entry for the gradient), against
``gpry_loo`` (the same q, hence rounding of N terms and no more), its repeatability, the not-positive-definite convention,
the state contract of tests/test_ctx_state*, and ``fit_gpr_hyperparameters(objective="loo")``.

Shapes, the smallest at which each piece can go wrong: (50, 1) one partly filled tile; (130, 2) first size past 128, two tile
rows; (200, 3); (333, 5) 384 padded rows, d between the traces' width classes; (300, 17) width class 24; (256, 32) largest
d, no padding; (1100, 8) many tiles, split-K / stream-K products.
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loo_fit_model as lf  # noqa: E402

pytestmark = pytest.mark.gpu

W = 0x10
Y_MEAN, Y_STD = 0.3, 1.7

CASES = [(N, d, kid, white) for (N, d) in [(50, 1), (130, 2), (200, 3), (333, 5)] for kid in range(4) for white in (False, True)]
CASES += [(300, 17, 2, True), (256, 32, 0, False), (1100, 8, 3, True)]
IDS = [f"n{N}_d{d}_k{kid}{'_w' if white else ''}" for N, d, kid, white in CASES]


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


def load(dev, N, d, kid, white):
    X_, y_, a, theta = lf.problem(N, d, seed=N + d, white=white)
    dev.set_train(X_, y_, a)
    dev.set_theta(kid | W if white else kid, theta)
    dev.set_affine(None, None, Y_MEAN, Y_STD)
    return X_, y_, a, theta


_cache = {}


def evaluated(dev, case):
    """Everything the tests of one model need, computed once: the device's answers and the two numpy formulations."""
    if case in _cache:
        return _cache[case]
    N, d, kid, white = case
    X_, y_, a, theta = load(dev, *case)
    r = dict(theta=theta, y_=y_)
    r["grad"] = dev.loo_objective(theta, True)
    r["value"] = dev.loo_objective(theta, False)
    r["again"] = dev.loo_objective(theta, True)
    assert dev.factorize() == 0
    r["loo"] = dev.loo()
    r["a"] = lf.loo_explicit(X_, y_, a, theta, kid, white)
    r["b"] = lf.loo_one_product(X_, y_, a, theta, kid, white)
    _cache[case] = r
    return r


def bounds(r, N):
    """(value, gradient) deviations allowed: ten times (a) against (b), not below the LML's bounds on the same chain."""
    (va, ga), (vb, gb) = r["a"], r["b"]
    big = np.max(np.abs(gb))
    return max(10 * abs(va - vb), 1e-10 * (abs(vb) + N)), max(10 * np.max(np.abs(ga - gb)), 1e-7 * big)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_value_and_gradient_against_the_closed_form(dev, case):
    N, d, kid, white = case
    r = evaluated(dev, case)
    v, g, info = r["grad"]
    vb, gb = r["b"]
    tol_v, tol_g = bounds(r, N)
    big = np.max(np.abs(gb))
    print(f"loo_fit {IDS[CASES.index(case)]}: value dev {abs(v - vb) / (abs(vb) + N):.2e} of |ref| + N (a-b "
          f"{abs(r['a'][0] - vb) / (abs(vb) + N):.2e}); grad dev {np.max(np.abs(g - gb)) / big:.2e} of the largest entry "
          f"(a-b {np.max(np.abs(r['a'][1] - gb)) / big:.2e})")
    assert info == 0 and g.shape == (d + 1 + int(white),)
    assert abs(v - vb) <= tol_v
    assert np.max(np.abs(g - gb)) <= tol_g


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_value_is_the_sum_of_gpry_loo_log_densities(dev, case):
    N = case[0]
    r = evaluated(dev, case)
    y = r["y_"] * Y_STD + Y_MEAN
    mean, var = r["loo"]["mean"], r["loo"]["var_y"]
    terms = np.concatenate([-0.5 * np.log(2 * np.pi * var), -0.5 * (y - mean) ** 2 / var, np.full(N, math.log(Y_STD))])
    total = float(np.sum(terms))
    print(f"loo_fit {IDS[CASES.index(case)]}: value - sum of gpry_loo densities {abs(total - r['grad'][0]):.2e}, "
          f"allowed {1e-11 * (np.sum(np.abs(terms)) + N):.2e}")
    assert abs(total - r["grad"][0]) <= 1e-11 * (np.sum(np.abs(terms)) + N)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_bits_with_and_without_gradient_and_on_a_second_call(dev, case):
    r = evaluated(dev, case)
    assert r["value"] == (r["grad"][0], 0)
    assert r["again"][0] == r["grad"][0] and np.array_equal(r["again"][1], r["grad"][1]) and r["again"][2] == 0


@pytest.mark.parametrize("case", [(130, 2, 1, True), (333, 5, 3, False), (1100, 8, 3, True)])
def test_same_bits_on_a_second_context(dev, case):
    from gpry_amd import _lib
    r = evaluated(dev, case)
    other = _lib.Device(0)
    try:
        load(other, *case)
        v, g, info = other.loo_objective(r["theta"], True)
    finally:
        other.close()
    assert info == 0 and v == r["grad"][0] and np.array_equal(g, r["grad"][1])


@pytest.mark.parametrize("N,d,kid", [(64, 2, 0), (200, 3, 3)])
def test_not_positive_definite_and_the_call_after_it(dev, N, d, kid):
    X_, y_, a, theta = lf.problem(N, d, seed=N + d, white=False)
    Xd = X_.copy()
    Xd[N // 2:] = Xd[:N - N // 2]                     # every row twice, no noise
    dev.set_train(Xd, y_, np.zeros(N))
    dev.set_theta(kid, theta)
    v, g, info = dev.loo_objective(theta, True)
    assert v == -np.inf and not g.any() and info > 0
    assert dev.loo_objective(theta, False) == (-np.inf, info)
    dev.set_train(X_, y_, a)
    v, g, info = dev.loo_objective(theta, True)
    vb, gb = lf.loo_one_product(X_, y_, a, theta, kid, False)
    assert info == 0 and abs(v - vb) <= 1e-10 * (abs(vb) + N) and np.max(np.abs(g - gb)) <= 1e-7 * np.max(np.abs(gb))


def snapshot(dev, theta_other, Xq):
    """The answers of the other entry points, in a fixed order."""
    out = [dev.lml(theta_other, True)]
    assert dev.factorize() == 0
    out.append(dev.get_factor())
    out.append(dev.predict(Xq, return_std=True))
    loo = dev.loo()
    out.append([loo[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")])
    sw = dev.sweep_logexp(Xq, 1.0, 0.5, 0.01)
    out.append(sw[0] if isinstance(sw, tuple) else sw)
    return out


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("case", [(200, 3, 3, True), (1100, 8, 3, False)])
def test_every_other_entry_point_answers_as_if_the_call_had_not_been_made(dev, case):
    N, d, kid, white = case
    X_, y_, a, theta = load(dev, *case)
    Xq = np.random.default_rng(2).uniform(0, 1, (40, d))
    other, there = theta.copy(), theta.copy()
    other[:d + 1] += 0.1
    there[:d + 1] -= 0.15
    before = snapshot(dev, other, Xq)
    mean_before = dev.predict(Xq[:3])
    v, g, info = dev.loo_objective(there, True)
    assert info == 0 and np.isfinite(v)
    assert np.array_equal(dev.predict(Xq[:3]), mean_before)            # the factor held for prediction, straight away
    after = snapshot(dev, other, Xq)
    for k, (x, y) in enumerate(zip(before, after)):
        assert same_bits(x, y), k
    # the factor cache of gpry_lml: an evaluation at the model's theta, then the objective elsewhere (its H and M now sit
    # where that evaluation's L and V sat), then a factorisation -- which must not adopt them
    dev.lml(theta, True)
    dev.loo_objective(there, True)
    assert dev.factorize() == 0
    assert same_bits(dev.get_factor(), before[1])
    # ... and the other way round: the objective's own factor is never offered either
    dev.loo_objective(theta, True)
    assert dev.factorize() == 0
    assert same_bits(dev.get_factor(), before[1])


# ------------------------------------------------------------------------------------ the fit
def make_gpr():
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as C, WhiteKernel
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    b = np.array([[0.0, 1.0], [0.0, 1.0]])
    kernel = C(1.0, [1e-3, 1e4]) * RBF([1.0, 1.0], [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    return GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=3, noise_level=1e-2,
                                    preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                    account_for_inf=None, random_state=7)


@pytest.fixture(scope="module")
def fit_data():
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (120, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(120)


def test_lml_objective_and_default_are_the_fit_without_the_argument(fit_data):
    X, y = fit_data
    plain = make_gpr().append_to_data(X, y, fit_gpr=True)                       # fit_objective unset, no argument
    assert not hasattr(plain, "fit_objective") and plain.fit_stats["objective"] == "lml"
    for arg in ({"objective": "lml"}, {"objective": None}):
        g = make_gpr().append_to_data(X, y, fit_gpr=arg)
        assert np.array_equal(g.kernel_.theta, plain.kernel_.theta)
        assert g.log_marginal_likelihood_value_ == plain.log_marginal_likelihood_value_
        assert g.loo_value_ is None
        assert g.fit_stats.keys() == plain.fit_stats.keys()


def test_loo_fit_against_scipy_on_the_closed_form(fit_data):
    """The leave-one-out refit of the LML-fitted model: run 0 starts from the current theta (the reference's schedule) and
    L-BFGS-B never accepts a worse point, so it ends no lower by the leave-one-out value than the LML fit; and it ends
    where scipy ends on the numpy closed form from the same three starts."""
    import scipy.optimize
    from gpry_amd.tools import check_random_state
    X, y = fit_data
    g = make_gpr().append_to_data(X, y, fit_gpr=True)
    theta_lml = g.kernel_.theta.copy()
    at_lml = g.loo_log_predictive(theta_lml)
    hb = g.kernel_.bounds
    g.fit_gpr_hyperparameters(objective="loo")
    assert g.fit_stats["objective"] == "loo" and g.fit_stats["side_by_side"] is False and g.fit_stats["why"]
    assert g.loo_value_ >= at_lml
    assert g.loo_log_predictive() == g.loo_value_
    assert g.log_marginal_likelihood_value_ == g.log_marginal_likelihood(g.kernel_.theta)
    # formulation (b) from the same starts: the current theta, then the reference's draws
    rng = check_random_state(7)
    starts = [theta_lml] + [rng.uniform(hb[:, 0], hb[:, 1]) for _ in range(2)]
    X_, y_, a = g.X_train_, g.y_train_, np.broadcast_to(g.alpha, (len(y),))

    def f(th):
        v, gr = lf.loo_one_product(X_, y_, a, th, 0, True)
        return -v, -gr
    runs = [scipy.optimize.minimize(f, s, method="L-BFGS-B", jac=True, bounds=hb) for s in starts]
    best = -min(r.fun for r in runs)
    th_best = runs[int(np.argmin([r.fun for r in runs]))].x
    va, ga = lf.loo_explicit(X_, y_, a, th_best, 0, True)
    vb, gb = lf.loo_one_product(X_, y_, a, th_best, 0, True)
    tol = max(10 * abs(va - vb), 1e-10 * (abs(vb) + len(y)))
    print(f"loo_fit fit: device {g.loo_value_!r} at {g.kernel_.theta}, scipy on the closed form {best!r} at {th_best}, "
          f"difference {abs(g.loo_value_ - best):.2e}, allowed {tol:.2e}; LML fit's theta gives {at_lml!r}")
    assert abs(g.loo_value_ - best) <= tol


def test_value_is_gpr_loo_log_densities(fit_data):
    """The regressor's own ``loo()`` (units of y) against its ``loo_log_predictive`` (transformed units)."""
    X, y = fit_data
    g = make_gpr().append_to_data(X, y, fit_gpr={"objective": "loo", "n_restarts": 1})
    loo = g.loo()
    std_y = float(g.preprocessing_y.std_)
    terms = np.concatenate([-0.5 * np.log(2 * np.pi * loo["var_y"]), -0.5 * (g.y_train - loo["mean"]) ** 2 / loo["var_y"],
                            np.full(len(y), math.log(std_y))])
    assert abs(float(np.sum(terms)) - g.loo_value_) <= 1e-11 * (np.sum(np.abs(terms)) + len(y))
