"""``C * (RBF | Matern) + WhiteKernel`` without a GPU: the kernel algebra against golden vectors of the reference
(tests/golden/white_noise.npz, tools/make_goldens_white.py), the numpy closed form the GPU tests compare with
(tests/tools/white_model.py) against the same vectors, and the regressor's host logic on the numpy stand-in of the device.
Tolerances: those of test_oracle_golden.py (kernel values 1e-13, LML 1e-10, gradient 1e-7 of its largest entry, mean
1e-8 / 1e-9, std 1e-6 / 1e-9).
"""
import copy
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import white_model as wm  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd.kernels import RBF, ConstantKernel as C, KERNEL_WHITE, Matern, Product, Sum, WhiteKernel  # noqa: E402

CASES = [(kid, s) for kid in range(4) for s in range(2)]
NU = {1: 0.5, 2: 1.5, 3: 2.5}


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-300))


def golden_kernel(kid, d, white_first=False, noise_bounds=(1e-6, 1e2)):
    """The kernel of the goldens (tools/make_goldens_white.py: white_kernel), before theta is set."""
    stat = RBF([1.0] * d, [1e-3, 10.]) if kid == 0 else Matern([1.0] * d, [1e-3, 10.], nu=NU[kid])
    prod, white = C(1.0, [1e-4, 1e6]) * stat, WhiteKernel(1.0, noise_bounds)
    return white + prod if white_first else prod + white


@pytest.fixture(scope="module")
def g():
    return load_golden("white_noise")


# ------------------------------------------------------------------------------------ kernel algebra
@pytest.mark.parametrize("kid,s", CASES)
def test_kernel_algebra_vs_reference(g, kid, s):
    p = f"k{kid}_s{s}_"
    theta, d = g[p + "theta"], g[p + "X_"].shape[1]
    k = golden_kernel(kid, d)
    assert isinstance(k, Sum) and isinstance(k.k1, Product) and isinstance(k.k2, WhiteKernel)
    k.theta = theta
    np.testing.assert_allclose(k.theta, theta, rtol=1e-15, atol=1e-15)
    np.testing.assert_array_equal(k.bounds, g[p + "theta_bounds"])
    assert repr(k) == str(g[p + "repr"]) and repr(k).endswith("+ WhiteKernel(noise_level=0.05)")
    np.testing.assert_allclose(k.diag(g[p + "X_"][:16]), g[p + "diag"], rtol=1e-15)     # C + w
    assert k.n_dims == d + 2 and [h.name for h in k.hyperparameters] == \
        ["k1__k1__constant_value", "k1__k2__length_scale", "k2__noise_level"]
    assert set(k.get_params()) >= {"k1", "k2", "k1__k1__constant_value", "k2__noise_level", "k2__noise_level_bounds"}
    kid_dev, full = k.device_spec(d)
    assert kid_dev == (kid | KERNEL_WHITE)
    np.testing.assert_allclose(full, theta, rtol=1e-15, atol=1e-15)
    # clone_with_theta leaves the original alone; the fast path of the objective agrees with the setter
    th2 = theta + 0.25
    c = k.clone_with_theta(th2)
    np.testing.assert_allclose(c.theta, th2, rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(k.theta, theta, rtol=1e-15, atol=1e-15)
    kid2, full2 = copy.deepcopy(k).set_theta_and_full(th2, d)
    assert kid2 == kid_dev
    np.testing.assert_array_equal(full2, c.device_spec(d)[1])
    gf = np.arange(1.0, d + 3.0)
    np.testing.assert_array_equal(k.grad_from_full(gf, d), gf)
    np.testing.assert_array_equal(k.grad_from_full_fast(gf, d), gf)
    assert k.plain_theta(d)
    # deep copy and pickle round trip
    for k2 in (copy.deepcopy(k), pickle.loads(pickle.dumps(k))):
        assert repr(k2) == repr(k)
        np.testing.assert_array_equal(k2.theta, k.theta)
        np.testing.assert_array_equal(k2.bounds, k.bounds)
    assert not np.any(k.k2.gradient_x(g[p + "X_"][0], g[p + "X_"]))


def test_operand_order_and_fixed_bounds(g):
    p = "k3_s0_"
    theta, d = g[p + "theta"], 2
    k = golden_kernel(3, d, white_first=True)
    assert isinstance(k.k1, WhiteKernel)
    k.theta = np.append(theta[-1:], theta[:-1])              # theta follows the operands: log w first
    np.testing.assert_allclose(k.device_spec(d)[1], theta, rtol=1e-15, atol=1e-15)      # the device vector does not
    assert k.device_spec(d)[0] == (3 | KERNEL_WHITE)
    np.testing.assert_array_equal(k.bounds, np.vstack([g[p + "theta_bounds"][-1:], g[p + "theta_bounds"][:-1]]))
    assert repr(k).startswith("WhiteKernel(noise_level=0.05) + ")
    gf = np.arange(1.0, d + 3.0)
    np.testing.assert_array_equal(k.grad_from_full(gf, d), np.append(gf[-1:], gf[:-1]))
    np.testing.assert_array_equal(k.grad_from_full_fast(gf, d), np.append(gf[-1:], gf[:-1]))
    assert not k.plain_theta(d)
    kid2, full2 = k.set_theta_and_full(np.append(theta[-1:], theta[:-1]) + 0.5, d)
    np.testing.assert_allclose(full2, theta + 0.5, rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(k.diag(np.zeros((3, d))), np.exp(theta[0] + 0.5) + np.exp(theta[-1] + 0.5), rtol=1e-15)
    # "fixed": the entry leaves theta and the gradient, w stays in the model
    kf = golden_kernel(3, d, noise_bounds="fixed")
    kf.k2.noise_level = 0.05
    assert kf.n_dims == d + 1 and kf.bounds.shape == (d + 1, 2)
    kf.theta = theta[:-1]
    np.testing.assert_allclose(kf.device_spec(d)[1], theta, rtol=1e-15, atol=1e-15)
    np.testing.assert_array_equal(kf.grad_from_full(gf, d), gf[:-1])
    np.testing.assert_array_equal(kf.grad_from_full_fast(gf, d), gf[:-1])
    assert kf.set_theta_and_full(theta[:-1] + 0.1, d)[1][-1] == np.log(0.05)
    assert kf.clone_with_theta(theta[:-1]).k2.noise_level == 0.05
    # numbers take the reference's meaning: a ConstantKernel
    s = 2.0 + RBF(1.0)
    assert isinstance(s, Sum) and isinstance(s.k1, C) and s.k1.constant_value == 2.0
    s = RBF(1.0) + 2.0
    assert isinstance(s.k2, C) and repr(s) == "RBF(length_scale=1) + 1.41**2"


@pytest.mark.parametrize("bad", ["rbf+rbf", "white", "prod+const", "const*sum"])
def test_refused_kernels_keep_todays_wording(bad):
    prod = C(2.0) * RBF([1.0, 1.0])
    k = {"rbf+rbf": RBF(1.0) + RBF(2.0), "white": WhiteKernel(0.1), "prod+const": prod + 2.0,
         "const*sum": C(2.0) * (RBF(1.0) + WhiteKernel(0.1))}[bad]
    with pytest.raises(NotImplementedError, match="run on the device"):
        k.device_spec(2)


# ------------------------------------------------------------------------------------ the closed form
@pytest.mark.parametrize("kid,s", CASES)
def test_closed_form_vs_reference(g, kid, s):
    p = f"k{kid}_s{s}_"
    X_, y_, alpha, theta = g[p + "X_"], g[p + "y_"], g[p + "alpha"], g[p + "theta"]
    K = wm.kernel_train(X_, theta, kid)
    if s == 0:
        np.testing.assert_allclose(K, g[p + "K"], rtol=1e-13, atol=0)
    else:
        np.testing.assert_allclose(K[:16], g[p + "K_rows"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(np.diag(K), g[p + "K_diag"], rtol=1e-13, atol=0)
    lml, grad = wm.lml(X_, y_, alpha, theta, kid, eval_gradient=True)
    assert abs(lml - g[p + "lml"]) <= 1e-10 * abs(g[p + "lml"])
    assert abs(wm.lml(X_, y_, alpha, theta, kid) - g[p + "lml_nograd"]) <= 1e-10 * abs(g[p + "lml"])
    assert grad.shape == (X_.shape[1] + 2,) and relmax(grad, g[p + "grad"]) < 1e-7
    b = g[p + "bounds"]
    m = wm.WhiteModel(X_, y_, alpha, kid, theta, b[:, 0], b[:, 1] - b[:, 0], g[p + "y_mean"], g[p + "y_std"])
    assert abs(wm.white_grad_from_factor(m.V, m.alpha_, m.w) - g[p + "grad"][-1]) <= 1e-7 * np.max(np.abs(g[p + "grad"]))
    Xc = g[p + "Xc"]
    mean, std = m.predict(Xc)
    np.testing.assert_allclose(mean, g[p + "mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(std, g[p + "std"], rtol=1e-6, atol=1e-9)
    sigma_n = float(np.mean(g[p + "noise_level"]))
    acq = m.logexp(Xc, float(g[p + "zeta"]), float(np.max(g[p + "y"])), sigma_n)
    np.testing.assert_allclose(acq, g[p + "acq"], rtol=1e-6, atol=1e-6)
    if kid != 1:
        for x, mg, sg in zip(Xc, g[p + "mean_grad"], g[p + "std_grad"]):
            mg1, sg1 = m.predict_grad(x)
            np.testing.assert_allclose(mg1, mg, rtol=1e-8, atol=1e-8 * np.max(np.abs(g[p + "mean_grad"])))
            np.testing.assert_allclose(sg1, sg, rtol=1e-6, atol=1e-8 * np.max(np.abs(g[p + "std_grad"])))


# ------------------------------------------------------------------------------------ the regressor on the stand-in
def make_gpr(g, p, kid):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import clone
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    bounds, d = g[p + "bounds"], g[p + "X_"].shape[1]
    gpr = attach(GaussianProcessRegressor(kernel=golden_kernel(kid, d), bounds=bounds, noise_level=1e-2, optimizer=None,
                                          preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(),
                                          account_for_inf=None), wm.WhiteDevice())
    k = clone(gpr.kernel)
    k.theta = g[p + "theta"]
    gpr.kernel_, gpr._fitted = k, True
    return gpr


@pytest.mark.parametrize("kid", [0, 3])
def test_regressor_lml_predict_and_border_append(g, kid):
    p = f"k{kid}_s0_"
    X, y, theta, Xc = g[p + "X"], g[p + "y"], g[p + "theta"], g[p + "Xc"]
    d = X.shape[1]
    gpr = make_gpr(g, p, kid)
    gpr.append_to_data(X[:36], y[:36], fit_gpr=False)
    gpr.append_to_data(X[36:], y[36:], fit_gpr=False, fit_classifier=False)       # the border path
    dev = gpr.device
    assert getattr(dev, "n_border", 0) == 1 and dev.white and dev.w == pytest.approx(0.05, rel=1e-14)
    assert dev.N == 40
    # (the y-preprocessor was fitted on the first 36 points: evaluate in ITS units)
    lml, grad = gpr.log_marginal_likelihood(theta, eval_gradient=True)
    assert grad.shape == (d + 2,)
    ref = wm.lml(gpr.X_train_, gpr.y_train_, gpr.alpha, theta, kid, eval_gradient=True)
    assert lml == pytest.approx(ref[0], rel=1e-12) and relmax(grad, ref[1]) < 1e-10
    assert gpr.log_marginal_likelihood(theta) == pytest.approx(ref[0], rel=1e-12)
    mean, std = gpr.predict(Xc, return_std=True)
    m = wm.WhiteModel(gpr.X_train_, gpr.y_train_, gpr.alpha, kid, theta, g[p + "bounds"][:, 0],
                      g[p + "bounds"][:, 1] - g[p + "bounds"][:, 0], gpr.preprocessing_y.mean_, gpr.preprocessing_y.std_)
    rm, rs = m.predict(Xc)
    np.testing.assert_allclose(mean, rm, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(std, rs, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gpr.predict_std(Xc), rs, rtol=1e-10, atol=1e-12)
    for x in Xc[:4]:
        m1, s1, mg, sg = gpr.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True)
        rmg, rsg = m.predict_grad(x)
        np.testing.assert_allclose(np.ravel(mg), rmg, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(np.ravel(sg), rsg, rtol=1e-7, atol=1e-10)
    # copies keep the term
    for c in (copy.deepcopy(gpr),):
        assert repr(c.kernel_) == repr(gpr.kernel_)
        np.testing.assert_allclose(c.predict(Xc, return_std=True)[1], std, rtol=1e-12)


def test_regressor_matches_reference_predictions(g):
    """All 40 points at once: the regressor's preprocessing is the golden's, so are mean, std and the LML."""
    p = "k2_s0_"
    gpr = make_gpr(g, p, 2)
    gpr.append_to_data(g[p + "X"], g[p + "y"], noise_level=g[p + "noise_level"], fit_gpr=False)
    np.testing.assert_allclose(gpr.alpha, g[p + "alpha"], rtol=1e-14)
    lml, grad = gpr.log_marginal_likelihood(g[p + "theta"], eval_gradient=True)
    assert abs(lml - g[p + "lml"]) <= 1e-10 * abs(g[p + "lml"]) and relmax(grad, g[p + "grad"]) < 1e-7
    mean, std = gpr.predict(g[p + "Xc"], return_std=True)
    np.testing.assert_allclose(mean, g[p + "mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(std, g[p + "std"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(gpr.scales[0], np.sqrt(np.exp(g[p + "theta"][0])) * g[p + "y_std"], rtol=1e-12)


def test_sequential_and_side_by_side_fit_learn_the_noise(g):
    """The fit moves w from its start to the data's (0.09 / std_y^2 within a factor 2) and ends no lower than the
    reference's own fit, on the stand-in, through both restart schedules."""
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    bounds, X, y = g["fit_bounds"], g["fit_X"], g["fit_y"]
    for lockstep in (False, True):
        kernel = C(1.0, [1e-3, 1e4]) * RBF([1.0, 1.0], [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
        np.testing.assert_allclose(kernel.theta, g["fit_theta0"], rtol=1e-15, atol=1e-15)
        gpr = attach(GaussianProcessRegressor(kernel=kernel, bounds=bounds, n_restarts_optimizer=int(g["fit_n_restarts"]),
                                              noise_level=1e-2, preprocessing_X=Normalize_bounds(bounds),
                                              preprocessing_y=Normalize_y(), account_for_inf=None, random_state=3),
                     wm.WhiteDevice())
        gpr.fit_lockstep = lockstep
        gpr.append_to_data(X, y, fit_gpr=True)
        assert gpr.fit_stats["side_by_side"] == (lockstep and gpr.fit_stats["why"] == "")
        w = float(np.exp(gpr.kernel_.theta[-1]))
        target = 0.09 / float(g["fit_y_std"]) ** 2
        assert target / 2 < w < 2 * target
        assert gpr.log_marginal_likelihood_value_ >= g["fit_lml"] - 1e-6 * abs(g["fit_lml"])
