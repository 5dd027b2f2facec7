"""``gpry_lml_hessian`` on the device: the Hessian of the log marginal likelihood in theta against the numpy closed form
(tests/tools/lml_hessian_model.py, formulation (b); the allowed deviation is ten times the disagreement of the two numpy
formulations on the same model, but not below 1e-7 of the largest entry, the project's bound for the gradient on this
chain: test_loo_fit_gpu.py, test_white_noise_gpu.py), value and gradient bit for bit against ``gpry_lml``, exact symmetry,
repeatability, the not-positive-definite convention, the state contract of tests/test_ctx_state*, the size limit, and
``gpr.lml_hessian`` / ``hyper_laplace`` on a fitted regressor.

Shapes, the smallest at which each piece can go wrong: (50, 1) one partly filled tile; (130, 2) first size past 128, two tile
rows; (200, 3); (333, 5) 384 padded rows, d between the width classes; (300, 17) width class 24, two coordinate blocks of
the Gram; (256, 32) largest d, no padding, three blocks of matrix indices in the pair traces; (1100, 8) many tiles
(split-K / stream-K products in the factor chain; its 648 tiles of the batched product are too many for a split); (600, 1)
640 padded rows and 25 tiles: the batched product itself split in two over k, through the split buffer and its reduction.

Deviations measured on an MI355X (of max|H|; in brackets the two numpy formulations against each other): the worst case is
n600_d1_k0 with 3.5e-10 (2.1e-10), then n130_d2_k0 with 7.2e-11 (2.9e-11) and n50_d1_k3 with 7.0e-11 (6.4e-11); the cases
with a white term stay below 5e-12 (profiles/lml_hessian.md).
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lml_hessian_model as hm  # noqa: E402

pytestmark = pytest.mark.gpu

W = 0x10
Y_MEAN, Y_STD = 0.3, 1.7
LIMIT = 4096

CASES = [(N, d, kid, white) for (N, d) in [(50, 1), (130, 2), (200, 3), (333, 5)] for kid in range(4) for white in (False, True)]
CASES += [(300, 17, 2, True), (256, 32, 0, False), (1100, 8, 3, True), (600, 1, 0, False)]
IDS = [f"n{N}_d{d}_k{kid}{'_w' if white else ''}" for N, d, kid, white in CASES]
TWICE = [(50, 1, 2, False), (333, 5, 3, True), (1100, 8, 3, True),
         (600, 1, 0, False)]      # (the batched product split over k, on a context that has seen nothing else)


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


def load(dev, N, d, kid, white):
    X_, y_, a, theta = hm.problem(N, d, seed=N + d, white=white)
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
    r = dict(theta=theta)
    r["hess"] = dev.lml_hessian(theta)
    r["lml"] = dev.lml(theta, True)
    r["again"] = dev.lml_hessian(theta)
    r["a"] = hm.hessian_explicit(X_, y_, a, theta, kid, white)
    r["b"] = hm.hessian_via_V(X_, y_, a, theta, kid, white)
    _cache[case] = r
    return r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hessian_against_the_closed_form(dev, case):
    N, d, kid, white = case
    r = evaluated(dev, case)
    H, Ha, Hb = r["hess"]["H"], r["a"][2], r["b"][2]
    big = np.max(np.abs(Hb))
    dev_ab, dev_h = np.max(np.abs(Ha - Hb)), np.max(np.abs(H - Hb))
    print(f"lml_hessian {IDS[CASES.index(case)]}: H dev {dev_h / big:.2e} of max|H| (a-b {dev_ab / big:.2e}), "
          f"device {r['hess']['device_ms']:.3f} ms")
    p = d + 1 + int(white)
    assert r["hess"]["info"] == 0 and H.shape == (p, p) and np.isfinite(H).all()
    assert dev_h <= max(10 * dev_ab, 1e-7 * big)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_value_and_gradient_have_the_bits_of_gpry_lml(dev, case):
    r = evaluated(dev, case)
    lml, grad, info = r["lml"]
    assert info == 0 and r["hess"]["lml"] == lml and np.array_equal(r["hess"]["grad"], grad)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_symmetric_to_the_last_bit_and_the_same_on_a_second_call(dev, case):
    r = evaluated(dev, case)
    H = r["hess"]["H"]
    assert np.array_equal(H, H.T)
    assert np.array_equal(r["again"]["H"], H) and r["again"]["lml"] == r["hess"]["lml"]
    assert np.array_equal(r["again"]["grad"], r["hess"]["grad"])


@pytest.mark.parametrize("case", TWICE)
def test_same_bits_on_a_second_context(dev, case):
    from gpry_amd import _lib
    r = evaluated(dev, case)
    other = _lib.Device(0)
    try:
        load(other, *case)
        o = other.lml_hessian(r["theta"])
    finally:
        other.close()
    assert o["info"] == 0 and o["lml"] == r["hess"]["lml"] and np.array_equal(o["grad"], r["hess"]["grad"])
    assert np.array_equal(o["H"], r["hess"]["H"])


def test_not_positive_definite_and_the_call_after_it(dev):
    theta = np.log([2.0, 0.3, 0.3])
    dev.set_train(np.zeros((6, 2)), np.arange(6.0), np.zeros(6))        # all rows equal, no noise
    dev.set_theta(0, theta)
    r = dev.lml_hessian(theta)
    assert r["lml"] == -np.inf and not r["grad"].any() and not r["H"].any() and r["info"] > 0
    assert r["grad"].shape == (3,) and r["H"].shape == (3, 3)
    # the same model through the chain alone (the single-launch objective is for d <= 16)
    case = (200, 3, 3, False)
    X_, y_, a, th = hm.problem(200, 3, seed=203, white=False)
    Xd = X_.copy()
    Xd[100:] = Xd[:100]
    dev.set_train(Xd, y_, np.zeros(200))
    dev.set_theta(3, th)
    r = dev.lml_hessian(th)
    assert r["lml"] == -np.inf and not r["grad"].any() and not r["H"].any() and r["info"] > 0
    good = evaluated(dev, case) if case in _cache else None
    load(dev, *case)
    r = dev.lml_hessian(th)
    Hb = hm.hessian_via_V(X_, y_, a, th, 3, False)[2]
    assert r["info"] == 0 and np.max(np.abs(r["H"] - Hb)) <= 1e-7 * np.max(np.abs(Hb))
    if good is not None:
        assert np.array_equal(r["H"], good["hess"]["H"])


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a if k != "device_ms")
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def snapshot(dev, theta_other, Xq, n_kb):
    """The answers of the other entry points on the factorised model with its Kriging-believer session, in a fixed order."""
    out = [dev.predict(Xq, return_std=True)]
    loo = dev.loo()
    out.append([loo[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")])
    out.append(dev.kb_gram(n_kb - 1, n_kb))
    out.append(dev.lml(theta_other, True))
    out.append(dev.loo_objective(theta_other, True))
    out.append(dev.kb_gram(0, n_kb))
    out.append(dev.predict(Xq, return_std=True))
    return out


@pytest.mark.parametrize("case", [(200, 3, 3, True), (1100, 8, 3, False)])
def test_every_other_entry_point_answers_as_if_the_call_had_not_been_made(dev, case):
    N, d, kid, white = case
    X_, y_, a, theta = load(dev, *case)
    Xq = np.random.default_rng(2).uniform(0, 1, (40, d))
    other, there = theta.copy(), theta.copy()
    other[:d + 1] += 0.1
    there[:d + 1] -= 0.15
    assert dev.factorize() == 0
    dev.kb_reset()
    n_kb = 5
    dev.kb_register(Xq[:n_kb])
    before = snapshot(dev, other, Xq, n_kb)
    factor = dev.get_factor()
    mean_before = dev.predict(Xq[:3])
    r = dev.lml_hessian(there)
    assert r["info"] == 0 and np.isfinite(r["H"]).all()
    assert np.array_equal(dev.predict(Xq[:3]), mean_before)            # the factor held for prediction, straight away
    after = snapshot(dev, other, Xq, n_kb)
    for k, (x, y) in enumerate(zip(before, after)):
        assert same_bits(x, y), k
    # the factor cache of gpry_lml: an evaluation at the model's theta, then the Hessian elsewhere (its scratch now holds
    # other matrices), then a factorisation -- which must not adopt them
    dev.lml(theta, True)
    dev.lml_hessian(there)
    assert dev.factorize() == 0
    assert same_bits(dev.get_factor(), factor)
    dev.lml_hessian(theta)
    assert dev.factorize() == 0
    assert same_bits(dev.get_factor(), factor)
    dev.kb_reset()


def test_a_model_above_the_limit_is_refused_before_anything_is_launched(dev):
    from gpry_amd._lib import GpryHipError
    N = LIMIT + 128
    rng = np.random.default_rng(1)
    X_ = rng.uniform(0, 1, (N, 1))
    theta = np.log([2.0, 0.3])
    dev.set_train(X_, np.sin(3 * X_[:, 0]), np.full(N, 1e-4))
    dev.set_theta(0, theta)
    dev.timing_reset()
    with pytest.raises(GpryHipError, match=str(LIMIT)):
        dev.lml_hessian(theta)
    for stage in ("kernel_build", "potrf", "solve_alpha", "lauum", "lml_traces", "hess_pairs", "hess_products", "hess_btraces",
                  "hess_middle", "hess_finish"):
        assert dev.timing(stage)[1] == 0, stage
    # the context answers the next call as before
    case = (130, 2, 1, True)
    X_, y_, a, th = load(dev, *case)
    r = dev.lml_hessian(th)
    Hb = hm.hessian_via_V(X_, y_, a, th, 1, True)[2]
    assert r["info"] == 0 and np.max(np.abs(r["H"] - Hb)) <= 1e-7 * np.max(np.abs(Hb))
    assert dev.timing("hess_products")[1] == 1
    if case in _cache:
        assert np.array_equal(r["H"], _cache[case]["hess"]["H"])


def test_bad_arguments_are_refused(dev):
    from gpry_amd._lib import GpryHipError
    X_, y_, a, theta = load(dev, 50, 1, 0, False)
    bad = theta.copy()
    bad[1] = np.nan
    with pytest.raises(GpryHipError, match="not finite"):
        dev.lml_hessian(bad)
    with pytest.raises(ValueError):
        dev.lml_hessian(theta[:1])
    assert dev.lml_hessian(theta)["info"] == 0


# ------------------------------------------------------------------------------------ the regressor
def test_gpr_lml_hessian_and_hyper_laplace_on_a_fitted_regressor():
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import Matern, ConstantKernel as C, WhiteKernel
    from gpry_amd.mc import hyper_laplace
    from gpry_amd.maximize import _inv_spd
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    N, d = 200, 3
    b = np.array([[0.0, 1.0]] * d)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(N)
    kernel = C(1.0, [1e-3, 1e4]) * Matern([1.0] * d, [1e-3, 10.], nu=2.5) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=3, noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=7)
    gpr.append_to_data(X, y, fit_gpr=True)
    gpr.fit_gpr_hyperparameters()
    theta = gpr.kernel_.theta.copy()
    n0 = gpr.n_eval_loglike
    lml, g, H = gpr.lml_hessian()
    assert gpr.n_eval_loglike == n0 + 1
    direct = gpr.device.lml_hessian(theta)
    assert lml == direct["lml"] and np.array_equal(g, direct["grad"]) and np.array_equal(H, direct["H"])
    l2, g2 = gpr.log_marginal_likelihood(theta, eval_gradient=True)
    assert lml == l2 and np.array_equal(g, g2)
    r = hyper_laplace(gpr)
    assert np.array_equal(r.H, H) and r.lml == lml and r.names == ["log C", "log l_1", "log l_2", "log l_3", "log w"]
    assert r.device_s > 0 and r.wall_s >= r.device_s
    # the same report from the numpy Hessian at that theta (it does not assume that the optimum is interior)
    lr, gr, Hr = hm.hessian_via_V(gpr.X_train_, gpr.y_train_, np.broadcast_to(gpr.alpha, (N,)), theta, 3, True)
    assert np.max(np.abs(H - Hr)) <= 1e-7 * np.max(np.abs(Hr))
    hb = np.asarray(gpr.kernel_.bounds)
    free = ~(np.isclose(theta, hb[:, 0], rtol=0, atol=1e-10) & (gr <= 0)) & ~(np.isclose(theta, hb[:, 1], rtol=0, atol=1e-10) & (gr >= 0))
    assert np.array_equal(r.free, free) and np.allclose(r.bounds, hb)
    inv = _inv_spd(-Hr[np.ix_(free, free)])
    assert r.negdef == (inv is not None)
    print(f"hyper_laplace: free {r.free}, negdef {r.negdef}, sigma_log {r.sigma_log}, log_evidence {r.log_evidence}")
    if inv is not None:
        assert np.max(np.abs(r.cov - inv[0])) <= 1e-6 * np.max(np.abs(inv[0]))
        assert np.max(np.abs(r.cov.dot(-H[np.ix_(free, free)]) - np.eye(int(free.sum())))) <= 1e-8
    else:
        assert r.cov is None
    if inv is not None and free.all():
        ev = lr + 0.5 * len(theta) * math.log(2 * math.pi) - 0.5 * inv[1] - float(np.sum(np.log(hb[:, 1] - hb[:, 0])))
        assert abs(r.log_evidence - ev) <= 1e-8 * abs(ev)
    else:
        assert math.isnan(r.log_evidence)
