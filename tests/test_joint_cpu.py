"""Joint posterior covariance, joint draws and their propagation, without a GPU: the numpy closed form of
tests/tools/joint_numpy.py against the oracle; ``predict(return_cov=True)`` and ``sample_y`` of the drop-in class on a numpy
device built from it (shapes, the ValueErrors, the unfitted prior, the 4096 limit, seeds); ``surrogate_spread`` of
gpry_amd/mc.py on hand-made cases with closed forms."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import joint_numpy as jn  # noqa: E402
import sampler_walk as sw  # noqa: E402


class NumpyDevice(jn.NumpyJoint, OracleDevice):
    """The oracle-backed device with the two joint calls."""


class InjectedDevice(NumpyDevice):
    """Draws f_s = mu + inject(X, S) (S x m) in place of the Gaussian ones."""
    inject = None

    def sample_joint(self, X, S, seed, jitter=None, mask=None, want_Z=False, want_Lc=False):
        mu, mean, _, _ = self._joint(X, mask)
        self.calls = getattr(self, "calls", 0) + 1
        return dict(mean=mean, Y=mu[None, :] + self.inject(np.asarray(X), int(S)), Z=None, Lc=None, jitter_used=0.0,
                    device_ms=0.0)


def _points(gpr, m, seed):
    rng = np.random.default_rng(seed)
    d = gpr.X_train.shape[1]
    X = rng.uniform(-3.0, 3.0, (m, d))
    X[: m // 2] = gpr.X_train[rng.choice(len(gpr.X_train), m // 2, replace=False)]
    return X


@pytest.mark.parametrize("kid,d,N,affine", [(sw.RBF, 2, 100, True), (sw.M32, 9, 300, False), (sw.M52, 17, 200, True),
                                            (sw.M12, 4, 150, False)])
def test_the_stand_in_covariance_against_the_oracle(kid, d, N, affine):
    model = sw.Model(d, kid, N, affine=affine, seed=N + d)
    ref = model.oracle()
    gpr = model.gpr(device=NumpyDevice())
    X = _points(gpr, 40, 1)
    S = jn.cov_of_oracle(ref, X)
    C = float(np.exp(model.theta[0]))
    y_std = float(ref.pre_y.inverse_transform_scale(np.ones(1))[0])
    _, std = ref.predict(X, return_std=True)
    free = std > 0                                  # (the oracle clamps a negative variance at 0)
    assert free.sum() >= 20
    np.testing.assert_allclose(np.diag(S)[free], std[free] ** 2, rtol=0, atol=1e-12 * C * y_std ** 2)
    np.testing.assert_array_equal(S, S.T)
    assert np.linalg.eigvalsh(S).min() >= -1e-9 * C * y_std ** 2
    # the longdouble variant is the same closed form: the float64 one lies within the products' rounding of it
    Sl = jn.cov_of_oracle(ref, X[:8], dtype=np.longdouble)
    assert np.max(np.abs(np.asarray(Sl - S[:8, :8], float))) <= 1e-9 * C * y_std ** 2
    # and the device built on it, through the class
    mean, cov = gpr.predict(X, return_cov=True)
    np.testing.assert_allclose(cov, S, rtol=0, atol=1e-12 * C * y_std ** 2)
    np.testing.assert_allclose(mean, ref.predict(X), rtol=0, atol=model.tol())


def test_predict_return_cov_and_sample_y_plumbing():
    model = sw.Model(3, sw.M52, 120, seed=4)
    gpr = model.gpr(device=NumpyDevice())
    X = _points(gpr, 10, 2)
    n0 = gpr.n_eval
    mean, cov = gpr.predict(X, return_cov=True)
    assert mean.shape == (10,) and cov.shape == (10, 10) and gpr.n_eval == n0 + 10
    for kw in (dict(return_std=True), dict(return_mean_grad=True), dict(return_std=True, return_mean_grad=True,
                                                                        return_std_grad=True)):
        with pytest.raises(ValueError, match="return_cov"):
            gpr.predict(X[:1], return_cov=True, **kw)
    big = np.zeros((4097, 3))
    with pytest.raises(ValueError, match="4096"):
        gpr.predict(big, return_cov=True)
    with pytest.raises(ValueError, match="4096"):
        gpr.sample_y(big)
    # every other branch of predict is as it was
    np.testing.assert_array_equal(gpr.predict(X), mean)
    m2, s2 = gpr.predict(X, return_std=True)
    np.testing.assert_allclose(s2 ** 2, np.clip(np.diag(cov), 0, None), rtol=0, atol=1e-12 * 4.0 * np.var(model.y))

    # draws: sklearn's orientation, one count per call, seeds
    n0 = gpr.n_eval
    Y = gpr.sample_y(X, n_samples=7, random_state=11)
    assert Y.shape == (10, 7) and gpr.n_eval == n0 + 10
    last = type(gpr).sample_y.last_result
    assert last["jitter_used"] == 1e-10 and last["seed"] == 11 and "device_ms" in last
    np.testing.assert_array_equal(Y, gpr.sample_y(X, n_samples=7, random_state=11))
    np.testing.assert_array_equal(Y[:, :3], gpr.sample_y(X, n_samples=3, random_state=11))
    assert not np.array_equal(Y, gpr.sample_y(X, n_samples=7, random_state=12))
    assert gpr.sample_y(X).shape == (10, 1)
    for make in (np.random.default_rng, np.random.RandomState):
        a, b = gpr.sample_y(X, 2, make(5)), gpr.sample_y(X, 2, make(5))
        np.testing.assert_array_equal(a, b)
        assert 0 <= type(gpr).sample_y.last_result["seed"] < 2 ** 63
    with pytest.raises(ValueError, match="n_samples"):
        gpr.sample_y(X, n_samples=0)
    # the draws are centred on the mean with the covariance's spread
    Yl = gpr.sample_y(X, n_samples=4000, random_state=3)
    far = np.diag(cov) > 1e-6
    assert np.all(np.abs(Yl.mean(axis=1) - mean)[far] <= 5 * np.sqrt(np.diag(cov)[far] / 4000))


def test_an_unfitted_model_returns_the_prior(monkeypatch):
    import gpry_amd.gpr as gpr_mod
    from gpry_amd.gpr import GaussianProcessRegressor
    from oracle import gpry_oracle as orc

    class Scratch(OracleDevice):        # the kernel object evaluates itself on a scratch context
        def kernel_train(self, add_alpha=False):
            return orc.kernel_matrix(self.X_, self.theta, self.kid)
    scratch = Scratch()
    monkeypatch.setattr(gpr_mod, "_scratch_device", lambda: scratch)
    bounds = np.array([[-1.0, 1.0]] * 2)
    gpr = GaussianProcessRegressor(kernel="RBF", bounds=bounds)
    X = np.random.default_rng(0).uniform(-1, 1, (5, 2))
    mean, cov = gpr.predict(X, return_cov=True)
    np.testing.assert_array_equal(mean, np.zeros(5))
    np.testing.assert_array_equal(cov, gpr.kernel(X))
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), gpr.predict(X, return_std=True)[1])


def test_the_stand_in_ladder_and_variates():
    Z = jn.normals(7, 5, 9)
    np.testing.assert_array_equal(Z[:3], jn.normals(7, 3, 9))
    np.testing.assert_array_equal(Z[:, :4], jn.normals(7, 5, 4))
    big = jn.normals(1, 400, 500)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1) < 5 * np.sqrt(2 / big.size)
    assert list(jn.ladder(0.0))[:3] == [0.0, 1e-14, 1e-12] and list(jn.ladder(None))[0] == 1e-10
    assert max(jn.ladder(0.0)) <= 1e-4
    S = np.array([[1.0, 1.0, 0.2], [1.0, 1.0, 0.2], [0.2, 0.2, 1.0]])       # an exact duplicate pair
    L, eps = jn.factor(S, 1.0, 0.0)
    assert eps > 0 and eps in list(jn.ladder(0.0)) and np.all(np.isfinite(L))
    assert jn.factor(np.eye(3), 1.0, 0.0)[1] == 0.0
    with pytest.raises(np.linalg.LinAlgError):
        jn.factor(-np.eye(2), 1.0, 0.0)


# ---- surrogate_spread -------------------------------------------------------------------------------------------------
def _spread_model(inject):
    model = sw.Model(1, sw.M52, 30, seed=5)
    dev = InjectedDevice()
    dev.inject = inject
    return model.gpr(device=dev)


def test_surrogate_spread_constant_offsets_move_log_z_and_nothing_else():
    from gpry_amd import mc
    c = np.random.default_rng(0).normal(0.0, 0.7, 64)
    gpr = _spread_model(lambda X, S: np.repeat(c[:S, None], len(X), axis=1))
    rng = np.random.default_rng(1)
    X = rng.normal(0.0, 1.0, (500, 1))
    w = rng.uniform(0.5, 1.5, 500)
    w[::7] = 0.0                                        # rows of zero weight are not sent to the device
    y = gpr.predict(X)
    before = mc.mc_sample_from_gp.last_result
    n0 = gpr.n_eval
    res = mc.surrogate_spread(gpr, X, y, w, n_draws=64, seed=3)
    assert mc.mc_sample_from_gp.last_result is before
    assert res.n_points == int((w > 0).sum()) and gpr.n_eval == n0 + res.n_points
    np.testing.assert_allclose(res.dlogZ, c, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.logZ_std, c.std(), rtol=1e-12)
    wn = w / w.sum()
    np.testing.assert_allclose(res.means, np.repeat([wn @ X], 64, axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.covs[:, 0, 0], wn @ (X[:, 0] - wn @ X[:, 0]) ** 2, rtol=1e-10)
    assert np.all(res.mean_shift_sigma < 1e-12) and np.all(res.cov_ratio_std < 1e-10)
    np.testing.assert_allclose(res.ess, 1.0 / np.sum(wn ** 2), rtol=1e-10)
    assert res.ess_min == res.ess.min() and res.jitter_used == 0.0


def test_surrogate_spread_tilts_shift_a_gaussian_sample_by_a_sigma_squared():
    from gpry_amd import mc
    a = np.linspace(-0.5, 0.5, 16)
    gpr = _spread_model(lambda X, S: a[:S, None] * X[None, :, 0])
    rng = np.random.default_rng(2)
    sigma = 0.8
    X = rng.normal(0.0, sigma, (4000, 1))
    y = gpr.predict(X)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = mc.surrogate_spread(gpr, X, y, None, n_draws=16, seed=1)
    assert res.n_points == 4000
    # E[x e^(a x)] / E[e^(a x)] = a sigma^2 for x ~ N(0, sigma^2); Monte Carlo error sigma / sqrt(ESS) per draw
    err = np.abs(res.means[:, 0] - a * sigma ** 2)
    assert np.all(err <= 5 * sigma / np.sqrt(res.ess)), (err, res.ess)
    # log E[e^(a x)] = a^2 sigma^2 / 2, error sd(e^(a x)) / (E sqrt(n)) <= 0.1
    assert np.all(np.abs(res.dlogZ - a ** 2 * sigma ** 2 / 2) <= 5 * 0.5 / np.sqrt(4000))
    assert res.mean_shift_sigma[0] > 0.2 and res.logZ_std > 0

    # the resampling branch: importance weights, 20000 rows down to 2000, weighted means within the Monte Carlo error
    Xb = rng.normal(0.3, 1.2 * sigma, (20000, 1))
    wb = np.exp(-0.5 * (Xb[:, 0] / sigma) ** 2 + 0.5 * ((Xb[:, 0] - 0.3) / (1.2 * sigma)) ** 2)
    wb /= wb.sum()
    calls = gpr.device.calls
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rs = mc.surrogate_spread(gpr, Xb, gpr.predict(Xb), wb, n_draws=16, seed=4, max_points=2000)
    assert gpr.device.calls == calls + 1 and 1000 < rs.n_points <= 2000
    assert abs(rs.mean0[0] - wb @ Xb[:, 0]) <= 5 * sigma / np.sqrt(2000)
    assert np.all(np.abs(rs.means[:, 0] - a * sigma ** 2) <= 5 * sigma / np.sqrt(rs.ess) + 5 * sigma / np.sqrt(2000))
    again = mc.surrogate_spread(gpr, Xb, gpr.predict(Xb), wb, n_draws=16, seed=4, max_points=2000)
    np.testing.assert_array_equal(again.means, rs.means)


def test_surrogate_spread_warns_when_the_effective_sample_size_collapses():
    from gpry_amd import mc
    gpr = _spread_model(lambda X, S: 12.0 * np.arange(1, S + 1)[:, None] * X[None, :, 0])
    X = np.random.default_rng(3).normal(0.0, 1.0, (600, 1))
    with pytest.warns(UserWarning, match="effective sample size"):
        res = mc.surrogate_spread(gpr, X, gpr.predict(X), n_draws=4, seed=0)
    assert res.ess_min < 0.05 * 600
    with pytest.raises(ValueError, match="n_draws"):
        mc.surrogate_spread(gpr, X, gpr.predict(X), n_draws=1)
    with pytest.raises(ValueError, match="max_points"):
        mc.surrogate_spread(gpr, X, gpr.predict(X), max_points=5000)
