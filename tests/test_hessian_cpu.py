"""Hessian of the surrogate's mean without a GPU: the closed form of tests/tools/hessian_numpy.py against central
differences of the oracle's gradient, and the host code of gpry_amd/maximize.py on it: laplace_gp (covariance, free set,
walls, saddles, evidence) and covmat="laplace" (the H0 of maximize_gp / profile_gp, the first proposal of the chain
samplers, the fallback with its warning, Matern 1/2 and unknown strings refused)."""
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hessian_numpy as hn  # noqa: E402
import maximize_numpy as mn  # noqa: E402
import sampler_walk as sw  # noqa: E402
from hmc_numpy import oracle_grad_x  # noqa: E402

from gpry_amd.maximize import _h0, _usable, hessian_gp, laplace_gp, maximize_gp, profile_gp  # noqa: E402
from gpry_amd.mc import mc_sample_from_gp  # noqa: E402

BOX = np.array([[-4.0, 4.0]] * 2)


# ---- the closed form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("d", [2, 5, 17])
@pytest.mark.parametrize("kid", [sw.RBF, sw.M32, sw.M52])
def test_stand_in_against_central_differences_of_the_oracle_gradient(kid, d, affine):
    """Central differences of the oracle's raw-coordinate mean gradient, step 1e-5 of the span: within 1e-6 of the
    largest entry of H (measured: 2e-8 at worst; the margin is for the step), except Matern 3/2 at training rows, where
    the third derivative jumps and the difference quotient is first-order (6e-5 measured): 1e-3.  H is exactly
    symmetric.  The stand-in's gradient is the oracle's up to the rounding of two orders of one sum."""
    model = sw.Model(d, kid, 100, affine=affine, seed=d + kid)
    ref = model.oracle()
    deriv = hn.MeanDerivatives.of_oracle(ref)
    grad = oracle_grad_x(ref)
    rng = np.random.default_rng(10 * d + kid)
    lo, hi = model.bounds[:, 0], model.bounds[:, 1]
    X = np.concatenate([rng.uniform(lo, hi, (5, d)), model.X[rng.choice(100, 3, replace=False)]])
    g, H = deriv.grad_hess(X)
    h = 1e-5 * (hi - lo)
    worst = [0.0, 0.0]
    for i, x in enumerate(X):
        fd = np.empty((d, d))
        for k in range(d):
            e = np.zeros(d)
            e[k] = h[k]
            fd[k] = (grad(x + e)[0] - grad(x - e)[0]) / (2 * h[k])
        err = np.max(np.abs(H[i] - fd)) / np.max(np.abs(H[i]))
        at_row = i >= 5
        worst[at_row] = max(worst[at_row], err)
        assert err <= (1e-3 if (at_row and kid == sw.M32) else 1e-6), (i, err)
        np.testing.assert_array_equal(H[i], H[i].T)
        # g is the oracle's sum in another order: both within N eps of the sum of the summands' magnitudes
        diff, aw, _ = deriv.terms(x)
        bound = 2 * 100 * np.finfo(float).eps * deriv.scale()[0] * (np.abs(aw) @ np.abs(diff)) / deriv.scale()[1]
        assert np.all(np.abs(g[i] - grad(x)[0]) <= bound), (i, np.abs(g[i] - grad(x)[0]) / bound)
    print(f"kid={kid} d={d} affine={affine}: worst relative error {worst[0]:.2e} (free points), {worst[1]:.2e} (training rows)")


def test_matern12_has_no_stand_in():
    with pytest.raises(ValueError, match="Matern-1/2"):
        hn.MeanDerivatives(np.zeros((3, 2)), np.zeros(3), np.zeros(3), sw.M12)


# ---- laplace_gp -------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(name="d=2"):
    """(HostGpr on the stand-in, MeanDerivatives) of an end-to-end model, made once: the tests read it only."""
    if name not in _ORACLE:
        _ORACLE[name] = hn.oracle_gpr(sw.Model(**mn.E2E_MODELS[name]))
    return _ORACLE[name]


def test_laplace_gp_covariance_evidence_and_counts_on_an_interior_maximum():
    gpr, deriv = _oracle()
    before = gpr.n_eval
    r = laplace_gp(gpr, nstarts=16)
    m = maximize_gp(gpr, nstarts=16)
    np.testing.assert_array_equal(r.x, m.x)
    lo, hi = gpr.bounds[:, 0], gpr.bounds[:, 1]
    assert np.all((r.x > lo) & (r.x < hi)) and r.free.all() and r.negdef
    g, H = deriv.grad_hess(r.x[None])
    np.testing.assert_array_equal(r.H, H[0])
    np.testing.assert_array_equal(r.g, g[0])
    assert r.y == float(gpr.device.loglike(r.x[None])[0])       # (the stand-in's y of the point alone)
    assert np.max(np.abs(r.cov @ (-r.H) - np.eye(2))) <= 1e-10
    logZ = r.y + np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(-r.H)[1] - np.sum(np.log(hi - lo))
    assert abs(r.logZ - logZ) <= 1e-12 * max(1.0, abs(logZ))
    assert gpr.n_eval - before == 2 * int(m.ncalls.sum()) + 1
    # a given x runs no maximisation, and takes none of its arguments
    r2 = laplace_gp(gpr, x=r.x)
    np.testing.assert_array_equal(r2.H, r.H)
    assert r2.logZ == r.logZ
    with pytest.raises(TypeError):
        laplace_gp(gpr, x=r.x, nstarts=4)
    with pytest.raises(ValueError):
        laplace_gp(gpr, x=hi + 1.0)
    # hessian_gp: the same numbers for a batch, n_eval by the number of points
    before = gpr.n_eval
    y, g3, H3 = hessian_gp(gpr, np.stack([r.x, lo, hi]))
    assert gpr.n_eval - before == 3 and y.shape == (3,) and g3.shape == (3, 2) and H3.shape == (3, 2, 2)
    np.testing.assert_array_equal(H3[0], r.H)
    with pytest.raises(ValueError):
        hessian_gp(gpr, np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError):
        hessian_gp(gpr, np.zeros((2, 3)))


def test_laplace_gp_leaves_a_fixed_coordinate_out():
    gpr, deriv = _oracle("d=3")
    r = laplace_gp(gpr, fixed=[1], nstarts=8)
    np.testing.assert_array_equal(r.free, [True, False, True])
    assert r.negdef and r.cov.shape == (2, 2) and np.isnan(r.logZ)
    Hff = r.H[np.ix_(r.free, r.free)]
    assert np.max(np.abs(r.cov @ (-Hff) - np.eye(2))) <= 1e-10


def test_laplace_gp_on_a_wall_with_an_outward_gradient():
    """The peak lies outside the box: the maximum is on the wall x_0 = 4 with g_0 > 0; that coordinate is not free and
    there is no evidence."""
    X = np.random.default_rng(0).uniform(BOX[:, 0], BOX[:, 1], (60, 2))
    gpr, q = hn.quadratic_gpr([5.0, 0.3], np.diag([1.0, 2.0]), BOX, X)
    r = laplace_gp(gpr, nstarts=8)
    assert r.x[0] == 4.0 and abs(r.x[1] - 0.3) < 1e-5 and r.g[0] > 0
    np.testing.assert_array_equal(r.free, [False, True])
    assert r.negdef and np.isnan(r.logZ)
    np.testing.assert_allclose(r.cov, [[0.5]], rtol=1e-12)
    # on the wall with the gradient pointing inward the coordinate stays free
    r = laplace_gp(gpr, x=[-4.0, 0.3])
    assert r.g[0] > 0 and r.free.all() and np.isfinite(r.logZ)


def test_laplace_gp_at_a_saddle_point():
    X = np.random.default_rng(0).uniform(BOX[:, 0], BOX[:, 1], (20, 2))
    gpr, q = hn.quadratic_gpr([0.3, 0.3], np.diag([1.0, -1.0]), BOX, X)
    r = laplace_gp(gpr, x=[0.3, 0.3])
    assert r.free.all() and not r.negdef and r.cov is None and np.isnan(r.logZ)
    np.testing.assert_array_equal(r.H, np.diag([-1.0, 1.0]))


# ---- covmat="laplace" -------------------------------------------------------------------------------------------------
def test_laplace_h0_is_the_inverse_of_minus_the_hessian_at_the_best_training_point():
    gpr, deriv = _oracle()
    dev = gpr.device
    lo, hi = gpr.bounds[:, 0], gpr.bounds[:, 1]
    span = hi - lo
    Xt, yt = _usable(gpr.X_train, gpr.y_train, lo, hi, gpr.minus_inf_value)
    H = deriv.grad_hess(Xt[:1])[1][0]
    want = np.linalg.inv(-H * np.outer(span, span))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = maximize_gp(gpr, nstarts=8, covmat="laplace")
        np.testing.assert_allclose(dev.calls[-1]["H0"], want, rtol=1e-10, atol=0)
        np.testing.assert_array_equal(dev.hess_calls[-1], Xt[:1])
        profile_gp(gpr, 0, [0.0, 0.3], nstarts=4, continuation=0, covmat="laplace")
        np.testing.assert_allclose(dev.calls[-1]["H0"], want, rtol=1e-10, atol=0)
    # not the default's H0, and the same maximum
    default = _h0(None, Xt, yt, span)
    assert np.max(np.abs(default - want)) > 1e-3 * np.max(np.abs(want))
    r0 = maximize_gp(gpr, nstarts=8)
    assert abs(r.y - r0.y) <= 1e-9 and r.n_distinct == r0.n_distinct


def test_laplace_h0_falls_back_with_a_warning_where_the_hessian_is_not_negative_definite():
    X = np.random.default_rng(0).uniform(BOX[:, 0], BOX[:, 1], (40, 2))
    gpr, q = hn.quadratic_gpr([0.3, 0.3], np.diag([1.0, -0.01]), BOX, X)
    Xt, yt = _usable(gpr.X_train, gpr.y_train, BOX[:, 0], BOX[:, 1], -np.inf)
    with pytest.warns(UserWarning, match="laplace"):
        maximize_gp(gpr, nstarts=4, covmat="laplace", max_iter=3)
    np.testing.assert_array_equal(gpr.device.calls[-1]["H0"], _h0(None, Xt, yt, BOX[:, 1] - BOX[:, 0]))


def _fake_runs(monkeypatch):
    """run_mcmc / run_hmc / run_tempered replaced by recorders of their keyword arguments."""
    seen = {}

    def fake(name):
        def run(dev, bounds, seed, n, X0, y0, **kw):
            seen[name] = kw
            return SimpleNamespace(X=np.zeros((1, len(bounds))), y=np.zeros(1), w=np.ones(1), ncalls=0, ngrad=0)
        return run
    import gpry_amd.hmc
    import gpry_amd.mcmc
    import gpry_amd.tempering
    monkeypatch.setattr(gpry_amd.mcmc, "run_mcmc", fake("mcmc"))
    monkeypatch.setattr(gpry_amd.hmc, "run_hmc", fake("hmc"))
    monkeypatch.setattr(gpry_amd.tempering, "run_tempered", fake("tempered"))
    return seen


@pytest.mark.parametrize("sampler", ["mcmc", "hmc", "tempered"])
def test_samplers_take_the_laplace_covariance_through_sampler_options(sampler, monkeypatch):
    seen = _fake_runs(monkeypatch)
    gpr, deriv = _oracle()
    cov = laplace_gp(gpr).cov
    mc_sample_from_gp(gpr, sampler=sampler, sampler_options={"covmat": "laplace"}, seed=1)
    np.testing.assert_array_equal(seen[sampler]["covmat"], cov)
    # a maximum on a wall has no such covariance: a warning, and the sampler's own default (None)
    X = np.random.default_rng(0).uniform(BOX[:, 0], BOX[:, 1], (60, 2))
    wall, _ = hn.quadratic_gpr([5.0, 0.3], np.diag([1.0, 2.0]), BOX, X)
    with pytest.warns(UserWarning, match="laplace"):
        mc_sample_from_gp(wall, sampler=sampler, sampler_options={"covmat": "laplace"}, seed=1)
    assert seen[sampler]["covmat"] is None
    with pytest.raises(ValueError, match="fisher"):
        mc_sample_from_gp(gpr, sampler=sampler, sampler_options={"covmat": "fisher"}, seed=1)


def test_matern12_raises_and_unknown_strings_are_still_refused(monkeypatch):
    _fake_runs(monkeypatch)
    gpr, deriv = hn.oracle_gpr(sw.Model(**mn.E2E_MODELS["d=2"]))
    for call in (lambda: maximize_gp(gpr, covmat="fisher"), lambda: profile_gp(gpr, 0, [0.0], covmat="fisher"),
                 lambda: maximize_gp(gpr, covmat="Laplace")):
        with pytest.raises(ValueError, match="covmat"):
            call()
    gpr.kernel_id = sw.M12
    for call in (lambda: maximize_gp(gpr, covmat="laplace"), lambda: profile_gp(gpr, 0, [0.0], covmat="laplace"),
                 lambda: laplace_gp(gpr), lambda: laplace_gp(gpr, x=[0.0, 0.0]), lambda: hessian_gp(gpr, np.zeros((1, 2))),
                 lambda: mc_sample_from_gp(gpr, sampler="mcmc", sampler_options={"covmat": "laplace"}),
                 lambda: mc_sample_from_gp(gpr, sampler="hmc", sampler_options={"covmat": "laplace"}),
                 lambda: mc_sample_from_gp(gpr, sampler="tempered", sampler_options={"covmat": "laplace"})):
        with pytest.raises(ValueError, match="Matern-1/2"):
            call()
    # without the option a Matern-1/2 model maximises as before
    assert np.isfinite(maximize_gp(gpr, nstarts=4, max_iter=2).y)
