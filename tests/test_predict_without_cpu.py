"""Predictions without a group of training points, without a GPU: the two numpy formulations of
tests/tools/predict_without_model.py against each other and against the leave-one-out formulas, ``gpr.predict_without`` on a
numpy device (``"last"``, ``"each"``, unsorted and overlapping groups, the refusals), and ``mc.batch_influence`` on synthetic
changes of the mean.

The bound between (a), the refit without the rows, and (b), the downdate from the full factor: both solve with K, whose
condition number on these models is 4e4 to 4e6 (noise 1e-4 to 1.1e-3 on a prior of 2, N up to 333), so each carries a forward
error of order cond(K) 2^-53 = 4e-10 relative to the size of the means (|y_| <= 3 y_std) and of the prior variance:
|a - b| <= 1e-8 max(1, 3 y_std) for the mean and 1e-8 C y_std^2 for the variance, a factor 25 above that estimate."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import loo_numpy as ln  # noqa: E402
import predict_without_model as wm  # noqa: E402
import sampler_walk as sw  # noqa: E402
import theta_grad_model as tm  # noqa: E402


class NumpyDevice(wm.NumpyWithout, ln.NumpyLoo, OracleDevice):
    """The oracle-backed device with the cross-validation calls and ``predict_without``."""


SMALL = [(50, 1, 1, False), (130, 2, 0, False), (130, 2, 1, True), (130, 2, 2, False), (130, 2, 3, True), (333, 5, 2, True)]


@pytest.mark.parametrize("case", SMALL)
def test_refit_and_downdate_agree_and_a_singleton_reproduces_leave_one_out(case):
    N, d, kid, white = case
    X_, y_, a, th = tm.problem(N, d, seed=N + d, white=white)
    Xq_ = tm.points(case, X_)
    C = math.exp(th[0])
    tol_m, tol_v = 1e-8 * max(1.0, 3.0 * tm.Y_STD), 1e-8 * C * tm.Y_STD ** 2
    for name, g in wm.groups_of(N):
        ma, va = wm.refit(X_, y_, a, th, kid, white, g, Xq_, tm.Y_STD)
        mb, vb = wm.downdate(X_, y_, a, th, kid, white, g, Xq_, tm.Y_STD)
        em, ev = np.max(np.abs(ma - mb)), np.max(np.abs(va - vb))
        print(f"n{N}_d{d}_k{kid}{'_w' if white else ''} {name}: |a - b| mean {em:.2e} (at {np.max(np.abs(ma)):.2e}), "
              f"var {ev:.2e} (at {np.max(np.abs(va)):.2e})")
        assert em <= tol_m and ev <= tol_v, (name, em, ev)
        assert np.all(vb >= 0.0) and np.all(va > -tol_v)
        # far outside the kernel row underflows: nothing changes
        assert np.all(mb[-2:] == 0.0) and np.all(vb[-2:] == 0.0)
        # the group as a set
        mp, vp = wm.downdate(X_, y_, a, th, kid, white, g[::-1], Xq_, tm.Y_STD)
        assert np.array_equal(mp, mb) and np.array_equal(vp, vb)
    # a singleton at its own row: mean + dmean = y_i - alpha_i / q_i and var + dvar = 1 / q_i - noise_i (transformed units)
    K, _ = tm._matrices(X_, a, th, kid, white)
    L = cholesky(K, lower=True)
    V = solve_triangular(L, np.eye(N), lower=True)
    al = V.T.dot(V.dot(y_))
    q = np.einsum("ki,ki->i", V, V)
    w = math.exp(th[d + 1]) if white else 0.0
    for i in (0, 5, N - 1):
        ks = wm._cross(X_, th, kid, X_[i:i + 1])
        mean0, expl0 = wm.full_model(K, y_, ks)
        for f in (wm.refit_K(K, y_, ks, [i]), wm.downdate_V(V, al, ks, [i])):
            assert abs(mean0[0] + f[0][0] - (y_[i] - al[i] / q[i])) <= 1e-8 * 3.0
            assert abs((C - expl0[0]) + f[1][0] - (1.0 / q[i] - (a[i] + w))) <= 1e-8 * C


def _model():
    model = sw.Model(3, sw.M52, 45, seed=4)
    full = sw.Model(3, sw.M52, 45, seed=4)
    model.X, model.y = full.X[:40], full.y[:40]
    gpr = model.gpr(device=NumpyDevice())
    gpr._ensure_factor()
    gpr.append_to_data(full.X[40:], full.y[40:], fit_gpr=False, fit_classifier=False)
    return model, gpr


def test_the_class_last_each_unsorted_overlapping_groups_and_the_refusals():
    from gpry_amd._lib import GpryHipError
    from gpry_amd.gpr import GaussianProcessRegressor
    model, gpr = _model()
    assert gpr.n_last_appended_finite == 5 and len(gpr.y_train) == 45
    Xs = np.random.default_rng(2).uniform(model.bounds[:, 0], model.bounds[:, 1], (7, 3))
    n0 = gpr.n_eval
    last = gpr.predict_without(Xs, "last")
    assert gpr.n_eval == n0 + 7 and len(last["groups"]) == 1 and last["dmean"].shape == last["dvar"].shape == (1, 7)
    np.testing.assert_array_equal(last["groups"][0], np.arange(40, 45))
    assert not last["info"].any() and np.all(last["dvar"] >= 0)
    # against a regressor that never saw the five points, at the same theta and pre-processors
    y_mean, y_std = gpr._y_affine()
    dev = gpr.device
    K = dev._factor[0].dot(dev._factor[0].T)
    from oracle import gpry_oracle as orc
    ks = orc.kernel_matrix(dev._to_unit(Xs), dev.theta, dev.kid, Y=dev.X_).T
    ma, va = wm.refit_K(K, dev.y_, ks, np.arange(40, 45), y_std)
    np.testing.assert_allclose(last["dmean"][0], ma, rtol=0, atol=1e-8 * max(1.0, np.max(np.abs(gpr.y_train))))
    np.testing.assert_allclose(last["dvar"][0], va, rtol=0, atol=1e-8 * y_std ** 2 * math.exp(dev.theta[0]))
    # unsorted and overlapping groups; a group listed twice
    res = gpr.predict_without(Xs, [[44, 40, 42, 41, 43], [40, 41, 42, 43, 44], [43, 3, 40], [3]])
    assert gpr.n_eval == n0 + 7 + 4 * 7
    np.testing.assert_array_equal(res["dmean"][0], res["dmean"][1])
    np.testing.assert_array_equal(res["dmean"][1], last["dmean"][0])
    np.testing.assert_array_equal(res["dvar"][0], last["dvar"][0])
    # "each": every training point alone, in order
    each = gpr.predict_without(Xs, "each")
    assert len(each["groups"]) == 45 and each["dmean"].shape == (45, 7)
    assert all(len(g) == 1 and g[0] == i for i, g in enumerate(each["groups"]))
    np.testing.assert_array_equal(each["dmean"][3], res["dmean"][3])
    # the model is as it was
    before = gpr.predict(Xs, return_std=True)
    gpr.predict_without(Xs, "each")
    after = gpr.predict(Xs, return_std=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for bad, word in (([[0, 1], []], "empty"), ([list(range(45)) + list(range(20))], "at most 64"), ([[0, 45]], "outside"),
                      ([[-1]], "outside"), ([[3, 7, 3]], "more than once")):
        with pytest.raises(GpryHipError, match=word):
            gpr.predict_without(Xs, bad)
    with pytest.raises(ValueError, match="each"):
        gpr.predict_without(Xs, "first")
    with pytest.raises(ValueError, match="last"):
        gpr.leave_out("each")                                # leave_out takes what it took
    with pytest.raises(ValueError, match="dimension"):
        gpr.predict_without(Xs[:, :2], "last")
    with pytest.raises(ValueError):
        gpr.predict_without(np.full((1, 3), np.nan), "last")
    empty = GaussianProcessRegressor(kernel="RBF", bounds=model.bounds)
    with pytest.raises(ValueError, match="training data"):
        empty.predict_without(Xs, [[0]])
    nothing = sw.Model(3, sw.M52, 30, seed=1).gpr(device=NumpyDevice())
    nothing.n_last_appended_finite = 0
    with pytest.raises(ValueError, match="no finite point"):
        nothing.predict_without(Xs, "last")
    with pytest.raises(GpryHipError, match="factor"):
        NumpyDevice().predict_without([[0]], Xs)


def test_the_wrapper_shares_the_group_arrays_with_leave_out():
    from gpry_amd._lib import Device
    ng, sizes, offsets, idx, ok = Device._group_arrays([[3, 1], [2], np.arange(5)])
    assert ng == 3 and ok and sizes.tolist() == [2, 1, 5] and offsets.tolist() == [0, 2, 3, 8]
    assert idx.tolist() == [3, 1, 2, 0, 1, 2, 3, 4] and idx.dtype == np.int64
    assert not Device._group_arrays([])[4] and not Device._group_arrays([[1], []])[4] and not Device._group_arrays([np.arange(65)])[4]


class FakeGpr:
    """``predict_without`` answering with given changes of the mean and of the variance."""

    def __init__(self, dmean, dvar=None, info=None):
        self.dmean = np.atleast_2d(np.asarray(dmean, dtype=float))
        self.dvar = np.zeros_like(self.dmean) if dvar is None else np.atleast_2d(np.asarray(dvar, dtype=float))
        self.info = np.zeros(len(self.dmean), dtype=np.int32) if info is None else np.asarray(info, dtype=np.int32)
        self.calls = []

    def predict_without(self, X, groups, validate=True):
        self.calls.append((np.array(X), groups))
        assert X.shape[0] == self.dmean.shape[1]
        g = [np.array([i]) for i in range(len(self.dmean))]
        return dict(dmean=self.dmean.copy(), dvar=self.dvar.copy(), info=self.info.copy(), groups=g, device_ms=0.25)


def test_batch_influence_constant_two_rows_rows_that_take_no_part_and_the_warning():
    from gpry_amd import mc
    rng = np.random.default_rng(0)
    n, d = 200, 3
    X = rng.standard_normal((n, d))
    y = -0.5 * (X ** 2).sum(1)
    w = rng.uniform(0.5, 1.5, n)
    # constant log r = c: dlogZ = c, kl = 0, ess and the moments are the sample's own
    c = 0.37
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = mc.batch_influence(FakeGpr(np.full((1, n), c), np.full((1, n), 0.5)), X, y, w)
    wn = w / w.sum()
    assert abs(r.dlogZ[0] - c) <= 1e-14 and abs(r.kl[0]) <= 1e-14 and abs(r.ess[0] - 1.0 / np.sum(wn * wn)) <= 1e-10
    np.testing.assert_allclose(r.means[0], wn.dot(X), rtol=0, atol=1e-14)
    np.testing.assert_allclose(r.covs[0], r.cov0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(r.mean_shift_sigma[0], 0.0, atol=1e-13)
    np.testing.assert_allclose(r.cov_ratio[0], 1.0, atol=1e-13)
    assert abs(r.max_abs_logr[0] - c) <= 1e-15 and abs(r.var_gain[0] - 0.5) <= 1e-14 and r.n_points == n and r.device_ms == 0.25
    assert not hasattr(r, "order") and "BatchInfluence" in repr(r)
    # two rows by hand: w = (1/4, 3/4), log r = (log 2, 0)
    X2 = np.array([[0.0], [4.0]])
    r = mc.batch_influence(FakeGpr([[math.log(2.0), 0.0]], [[1.0, 3.0]]), X2, np.zeros(2), np.array([1.0, 3.0]))
    Z = 0.25 * 2.0 + 0.75
    assert abs(r.dlogZ[0] - math.log(Z)) <= 1e-15
    assert abs(r.kl[0] - (math.log(Z) - 0.25 * math.log(2.0))) <= 1e-15 and r.kl[0] > 0
    p = np.array([0.5, 0.75]) / Z
    assert abs(r.ess[0] - 1.0 / np.sum(p * p)) <= 1e-14 and abs(r.means[0, 0] - 4.0 * p[1]) <= 1e-14
    assert abs(r.covs[0, 0, 0] - 16.0 * p[0] * p[1]) <= 1e-13 and abs(r.var_gain[0] - 2.5) <= 1e-15
    assert abs(r.mean_shift_sigma[0, 0] - abs(4.0 * p[1] - 3.0) / math.sqrt(3.0)) <= 1e-14
    assert abs(r.cov_ratio[0, 0] - 16.0 * p[0] * p[1] / 3.0) <= 1e-14
    # rows of zero weight or -inf y take no part: the device is asked for the others only
    w3 = w.copy()
    w3[[1, 5]] = 0.0
    y3 = y.copy()
    y3[[2, 9]] = -np.inf
    keep = np.setdiff1d(np.arange(n), [1, 2, 5, 9])
    lr = rng.normal(0, 0.3, (2, len(keep)))
    fake = FakeGpr(lr, np.abs(lr), info=[0, 3])
    r = mc.batch_influence(fake, X, y3, w3, groups="each")
    assert np.array_equal(r.keep, keep) and np.array_equal(fake.calls[0][0], X[keep]) and fake.calls[0][1] == "each"
    wk = w3[keep] / w3[keep].sum()
    assert abs(r.dlogZ[0] - math.log(np.sum(wk * np.exp(lr[0])))) <= 1e-14
    assert abs(r.kl[0] - (r.dlogZ[0] - wk.dot(lr[0]))) <= 1e-14 and r.kl[0] >= 0
    # a group whose block is not positive definite: NaN, and last in the order
    assert np.isnan(r.dlogZ[1]) and np.isnan(r.kl[1]) and np.isnan(r.means[1]).all() and r.info.tolist() == [0, 3]
    assert r.order.tolist() == [0, 1]
    # "each" orders by descending kl
    lr = np.stack([np.zeros(n), 0.5 * X[:, 0], 0.1 * X[:, 1]])
    r = mc.batch_influence(FakeGpr(lr), X, y, w, groups="each")
    assert r.order.tolist() == [1, 2, 0] and r.kl[1] > r.kl[2] > r.kl[0] - 1e-15
    # the 5 % warning
    spike = np.zeros((1, n))
    spike[0, 7] = 40.0
    with pytest.warns(UserWarning, match="5 %"):
        mc.batch_influence(FakeGpr(spike), X, y, w)
    with pytest.raises(ValueError, match="no row"):
        mc.batch_influence(FakeGpr(np.zeros((1, n))), X, np.full(n, -np.inf), w)
