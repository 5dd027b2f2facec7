"""``gpry_predict_thetas_var`` on the device: the predictive variance at M points under B thetas beside the mean, against the
numpy truth (tests/tools/predict_thetas_var_model.py), the bits contract, a theta that is not positive definite among good
ones, the state contract, the refusals, and ``hyper_predict`` end to end on a fitted regressor.

Shapes, thetas and points are tests/test_predict_thetas_gpu.py's (``pm.CASES``, ``pm.thetas_of``, ``tm.points``): 5 thetas,
26 points -- 8 training rows with a duplicated pair, 16 uniform, 2 far outside where k underflows and the variance is the
prior's, y_std^2 (C_b + w_b), exactly; 26 crosses a 16-column tile of the matrix pipe and, at Np = 128, no panel boundary
(64 points), which the chunk-boundary test does.

The bound against the closed form, per case and theta row: max_i |var_dev - var_a| <= max(10 max_i |var_a - var_b|, 2 D_seq),
var_a / var_b the two numpy formulations (a triangular solve / the explicit V = L^-1) and
D_seq = max_i |std_seq^2 - max(var_a, 0)| the deviation from (a) of the route that exists without this call -- set_theta +
factorize + predict(return_std=True) with the clip off and no gates -- on the same device in the same test:
test_predict_thetas_gpu.py's rule applied to the variance.  Also: var > -bound everywhere, and mean, lml and info have the
bits of the call without ``want_var``.

Measured on an MI355X (deviation / bound of the worst theta row; profiles/predict_thetas_var.md): n50_d1_k1 0.114; n130_d2
k0 0.422, k0_w 0.332, k1 0.167, k1_w 0.107, k2 0.400, k2_w 0.210, k3 0.672, k3_w 0.229; n333_d5_k2_w 0.217; n300_d17_k2_w
0.320; n256_d32_k0 0.500; n1100_d8_k3_w 0.111; n2500_d4_k1 0.153.  The deviations are 3.9e-16 to 5.3e-14 of the prior variance,
the smallest variance of a case is 2.6e-5 (no negative value occurs on these models); the end-to-end regressor has
|var0 - var_a| = 9.5e-16 against a bound of 1.2e-14.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict_thetas_model as pm  # noqa: E402
import predict_thetas_var_model as vm  # noqa: E402
import theta_grad_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def other():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


def setup(dev, case):
    """The case's model on ``dev``; (X_, y_, alpha, theta, thetas (5, p), Xq_ unit points, Xq raw points)."""
    X_, y_, a, th = tm.load(dev, case)
    Xq_ = tm.points(case, X_)
    return X_, y_, a, th, pm.thetas_of(case, th), Xq_, tm.to_raw(case, Xq_)


def flag(case):
    return case[2] | tm.W_FLAG if case[3] else case[2]


def prior(case, theta):
    """y_std^2 (C + w) as the library forms it: libm's exp, the sum, then the product with y_std * y_std."""
    return tm.Y_STD * tm.Y_STD * vm.prior_var(theta, case[1], case[3])


def var_of(dev, T, Xq):
    return dev.predict_thetas(T, Xq, want_var=True)["var"]


_ref = {}


def reference(case, X_, a, T, Xq_):
    """(var_a, var_b), each (5, 26), of the case: computed once and never changed."""
    if case not in _ref:
        N, d, kid, white = case
        va = np.stack([vm.var_numpy(X_, a, th, kid, white, Xq_, tm.Y_STD) for th in T])
        vb = np.stack([vm.var_via_V(X_, a, th, kid, white, Xq_, tm.Y_STD) for th in T])
        va.setflags(write=False)
        vb.setflags(write=False)
        _ref[case] = (va, vb)
    return _ref[case]


# ------------------------------------------------------------------------------------ against the closed form
@pytest.mark.parametrize("case", pm.CASES, ids=pm.IDS)
def test_var_against_the_closed_form_and_the_rest_with_the_bits_of_the_plain_call(dev, case):
    N, d, kid, white = case
    name = pm.IDS[pm.CASES.index(case)]
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    out = dev.predict_thetas(T, Xq, want_var=True)
    plain = dev.predict_thetas(T, Xq)
    assert out["var"].shape == (5, len(Xq)) and np.isfinite(out["var"]).all() and not out["info"].any() and out["device_ms"] > 0
    assert "var" not in plain
    for k in ("mean", "lml", "info"):
        assert np.array_equal(out[k], plain[k]), k
    # far outside k underflows: the prior variance exactly (with w for a model with a white term)
    for b in range(5):
        assert np.all(out["var"][b, -2:] == prior(case, T[b])), (b, out["var"][b, -2:], prior(case, T[b]))
    va, vb = reference(case, X_, a, T, Xq_)
    worst = 0.0
    try:
        for b in range(5):
            dev.set_theta(flag(case), T[b])
            assert dev.factorize() == 0
            seq = dev.predict(Xq, return_std=True)[1]
            ab = np.max(np.abs(va[b] - vb[b]))
            d_seq = np.max(np.abs(seq * seq - np.maximum(va[b], 0.0)))
            d_dev = np.max(np.abs(out["var"][b] - va[b]))
            bound = max(10.0 * ab, 2.0 * d_seq)
            print(f"predict_thetas_var {name} row {b}: deviation {d_dev:.3e} ({d_dev / prior(case, T[b]):.2e} of the prior variance), "
                  f"a-b {ab:.3e}, sequential route {d_seq:.3e}, min var {out['var'][b].min():.3e}, ratio {d_dev / bound:.3f}")
            worst = max(worst, d_dev / bound)
            assert d_dev <= bound, (b, d_dev, ab, d_seq)
            assert np.all(out["var"][b] > -bound), (b, out["var"][b].min(), bound)
    finally:
        tm.load(dev, case)
    print(f"predict_thetas_var {name}: worst ratio {worst:.3f}")


# ------------------------------------------------------------------------------------ bits
def two_sets_mb(dev):
    """``lml_batch_mb`` at which exactly two scratch sets of the last batched call's layout fit (test_predict_thetas_gpu.py)."""
    per_set = 8 * dev.timing("batch_set_doubles")[1]
    assert per_set > 0
    mb = -(-2 * per_set // (1 << 20))
    assert (mb << 20) // per_set == 2, (mb, per_set)
    return mb


@pytest.mark.parametrize("case", [(130, 2, 2, True), (1100, 8, 3, True)])
def test_same_bits_whatever_the_batch_the_position_the_chunking_the_route_and_the_context(dev, other, case):
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    whole = var_of(dev, T, Xq)
    assert np.array_equal(var_of(dev, T, Xq), whole)                                # a second call repeats the first
    assert dev.timing("batch_chunk")[1] == 5
    # rows permuted; one theta at a time (the one-after-another route)
    perm = np.array([4, 2, 0, 1, 3])
    assert np.array_equal(var_of(dev, T[perm], Xq), whole[perm])
    assert np.array_equal(np.vstack([var_of(dev, T[b:b + 1], Xq) for b in range(5)]), whole)
    # points permuted; one point at a time; 17 of them; the call split in two over thetas and over points
    pp = np.random.default_rng(1).permutation(len(Xq))
    assert np.array_equal(var_of(dev, T, Xq[pp]), whole[:, pp])
    assert np.array_equal(np.hstack([var_of(dev, T, Xq[i:i + 1]) for i in range(len(Xq))]), whole)
    assert np.array_equal(var_of(dev, T, Xq[:17]), whole[:, :17])
    assert np.array_equal(var_of(dev, T, Xq[9:]), whole[:, 9:])
    assert np.array_equal(np.vstack([var_of(dev, T[:2], Xq), var_of(dev, T[2:], Xq)]), whole)
    assert np.array_equal(np.hstack([var_of(dev, T, Xq[:11]), var_of(dev, T, Xq[11:])]), whole)
    keys = ("lml_batch_mb", "panel_debug", "lml_batch")
    keep = {k: dev.get_option(k) for k in keys}
    try:
        # exactly two sets fit: 2 + 2 + 1, every scratch set starting as NaNs
        dev.set_option("lml_batch_mb", two_sets_mb(dev))
        dev.set_option("panel_debug", keep["panel_debug"] | 128)
        assert np.array_equal(var_of(dev, T, Xq), whole)
        assert dev.timing("batch_chunk")[1] == 2
        dev.set_option("lml_batch_mb", keep["lml_batch_mb"])
        dev.set_option("panel_debug", keep["panel_debug"])
        # one after another
        dev.set_option("lml_batch", 0)
        assert np.array_equal(var_of(dev, T, Xq), whole)
    finally:
        for k in keys:
            dev.set_option(k, keep[k])
    # a second context
    tm.load(other, case)
    assert np.array_equal(var_of(other, T, Xq), whole)


def test_the_chunk_boundary_of_the_points(dev):
    case = (130, 2, 0, False)
    X_, y_, a, th, T, Xq_, Xq26 = setup(dev, case)
    M = 65536 + 5
    Xq = tm.to_raw(case, np.random.default_rng(5).uniform(0, 1, (M, 2)))
    at = np.concatenate([np.arange(65536 - 13, 65536 + 5), np.arange(8)])           # 18 across the boundary, 8 at the start
    Xq[at] = Xq26
    dev.timing_reset()
    out = dev.predict_thetas(T[:2], Xq, want_var=True)
    assert dev.timing("predict_thetas")[1] == 1 and dev.timing("predict_thetas_mean")[1] == 2
    assert dev.timing("predict_thetas_var")[1] == 2
    few = dev.predict_thetas(T[:2], Xq26, want_var=True)
    for j, i in enumerate(at):
        assert np.array_equal(out["var"][:, i], few["var"][:, j]), (j, i)
    assert np.array_equal(out["mean"][:, at], few["mean"]) and np.array_equal(out["mean"], dev.predict_thetas(T[:2], Xq)["mean"])
    # every column is a variance: between -rounding and the prior's
    for b in range(2):
        p = prior(case, T[b])
        assert np.all(out["var"][b] <= p) and np.all(out["var"][b] > -1e-9 * p)


# ------------------------------------------------------------------------------------ a theta that is not positive definite
@pytest.mark.parametrize("N,d,kid", [(100, 3, 0), (300, 5, 2)])
def test_a_theta_that_is_not_positive_definite_fails_on_its_own(dev, N, d, kid):
    """test_predict_thetas_gpu.py's construction: six duplicated training points, which every other theta survives thanks to
    the noise on their diagonal entries; at C = 1e15 that noise is below half an ulp of the diagonal."""
    rng = np.random.default_rng(7 * N + d + kid)
    X = rng.uniform(size=(N, d))
    y = np.sin(3 * X).sum(1) + 0.05 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    alpha = 1e-5 * (1.0 + rng.uniform(size=N))
    base = np.log(np.array([2.0] + [0.5] * d))
    T = base + rng.uniform(-0.7, 0.7, (5, d + 1))
    bad = 2
    for j in range(0, 12, 2):
        X[j + 1] = X[j]
    alpha[:12] = 1e-2
    T[bad, 0] = np.log(1e15)
    Xq = rng.uniform(size=(30, d))
    dev.set_train(X, y, alpha)
    dev.set_theta(kid, base)
    dev.set_affine(None, None, tm.Y_MEAN, tm.Y_STD)
    assert dev.factorize() == 0
    good = [b for b in range(5) if b != bad]
    without = dev.predict_thetas(T[good], Xq, want_var=True)
    assert not without["info"].any() and np.isfinite(without["var"]).all()
    out = dev.predict_thetas(T, Xq, want_var=True)
    assert out["info"][bad] > 0 and np.isneginf(out["lml"][bad]) and np.isnan(out["mean"][bad]).all() and np.isnan(out["var"][bad]).all()
    assert np.array_equal(out["var"][good], without["var"]) and np.array_equal(out["mean"][good], without["mean"])
    assert not out["info"][good].any()
    alone = dev.predict_thetas(T[bad:bad + 1], Xq, want_var=True)
    assert alone["info"][0] > 0 and np.isnan(alone["var"]).all()


# ------------------------------------------------------------------------------------ state
def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a if k != "device_ms")
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("case", [(50, 1, 1, False), (333, 5, 3, True), (1100, 8, 2, False)])
def test_no_other_entry_point_notices_the_call_and_the_call_notices_none_of_them(dev, other, case):
    N, d, kid, white = case
    X_, y_, a, th, T, Xq_, Xq = setup(other, case)
    fresh = other.predict_thetas(T, Xq, want_var=True)
    tm.load(dev, case)
    alt = th.copy()
    alt[:d + 1] += 0.1

    def loo():
        r = dev.loo()
        return [r[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")]
    ops = [("predict_std", lambda: dev.predict(Xq, return_std=True)), ("lml_grad", lambda: dev.lml(alt, True)), ("loo", loo),
           ("predict_1", lambda: dev.predict(Xq[:1])), ("mean_theta_grad", lambda: dev.mean_theta_grad(Xq))]
    before = [f() for _, f in ops]
    assert same_bits(dev.predict_thetas(T, Xq, want_var=True), fresh)
    after = [f() for _, f in ops]
    for (name, _), x, y in zip(ops, before, after):
        assert same_bits(x, y), name
    for name, f in ops:
        f()
        assert same_bits(dev.predict_thetas(T, Xq, want_var=True), fresh), name
    # the factor cache of gpry_lml: a factor adopted after the call is the theta's own
    dev.lml(T[1], True)
    dev.predict_thetas(T, Xq, want_var=True)
    dev.set_theta(flag(case), T[1])
    assert dev.factorize() == 0
    got = dev.predict(Xq, return_std=True)
    other.set_theta(flag(case), T[1])
    assert other.factorize() == 0
    assert same_bits(got, other.predict(Xq, return_std=True))


def test_a_white_term_is_part_of_the_variance(dev):
    case = (130, 2, 1, True)
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    var = var_of(dev, T, Xq)
    for b in range(5):
        w = math.exp(T[b][3])
        assert w > 0 and var[b, -1] == tm.Y_STD * tm.Y_STD * (math.exp(T[b][0]) + w) != tm.Y_STD * tm.Y_STD * math.exp(T[b][0])
        # at a training row the noise-free part is explained; what is left is at least most of w
        assert np.all(var[b, :8] > 0.5 * tm.Y_STD * tm.Y_STD * w)


def test_refusals_return_minus_one_with_a_message_and_the_context_answers_as_before(dev):
    from gpry_amd import _lib
    case = (130, 2, 1, True)
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    good = dev.predict(Xq, return_std=True)
    answer = dev.predict_thetas(T, Xq, want_var=True)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    X = np.ascontiguousarray(Xq[:2])
    Tc = np.ascontiguousarray(T[:3])
    mean, var, lml, info = np.empty((3, 2)), np.empty((3, 2)), np.empty(3), np.zeros(3, dtype=np.int32)
    xinf, xnan, tinf, tnan = X.copy(), X.copy(), Tc.copy(), Tc.copy()
    xinf[1, 0], xnan[0, 1], tinf[2, 1], tnan[0, 3] = np.inf, np.nan, -np.inf, np.nan
    for what, args, word in [("NULL thetas", (None, 3, vp(X), 2, vp(mean)), "NULL"), ("NULL X", (vp(Tc), 3, None, 2, vp(mean)), "NULL"),
                             ("NULL mean", (vp(Tc), 3, vp(X), 2, None), "NULL"), ("B 0", (vp(Tc), 0, vp(X), 2, vp(mean)), "B = 0"),
                             ("B < 0", (vp(Tc), -1, vp(X), 2, vp(mean)), "B = -1"), ("M 0", (vp(Tc), 3, vp(X), 0, vp(mean)), "M = 0"),
                             ("M < 0", (vp(Tc), 3, vp(X), -2, vp(mean)), "M = -2"),
                             ("x inf", (vp(Tc), 3, vp(xinf), 2, vp(mean)), "not finite"), ("x nan", (vp(Tc), 3, vp(xnan), 2, vp(mean)), "not finite"),
                             ("theta inf", (vp(tinf), 3, vp(X), 2, vp(mean)), "not finite"),
                             ("theta nan", (vp(tnan), 3, vp(X), 2, vp(mean)), "not finite")]:
        rc = dev._lib.gpry_predict_thetas_var(dev._h, *args, vp(var), vp(lml), vp(info), None)
        msg = dev._lib.gpry_last_error(dev._h).decode()
        assert rc == -1 and word in msg and "predict_thetas" in msg, (what, rc, msg)
        assert same_bits(dev.predict(Xq, return_std=True), good), what
    # var, lml, info and device_ms are optional; without var the call is gpry_predict_thetas
    assert dev._lib.gpry_predict_thetas_var(dev._h, vp(Tc), 3, vp(X), 2, vp(mean), vp(var), None, None, None) == 0
    assert np.array_equal(mean, answer["mean"][:3, :2]) and np.array_equal(var, answer["var"][:3, :2])
    mean[:] = 0.0
    assert dev._lib.gpry_predict_thetas_var(dev._h, vp(Tc), 3, vp(X), 2, vp(mean), None, None, None, None) == 0
    assert np.array_equal(mean, answer["mean"][:3, :2])
    assert same_bits(dev.predict(Xq, return_std=True), good) and same_bits(dev.predict_thetas(T, Xq, want_var=True), answer)
    # the wrapper's shape checks
    with pytest.raises(ValueError):
        dev.predict_thetas(T[:, :-1], Xq, want_var=True)
    with pytest.raises(ValueError):
        dev.predict_thetas(T, Xq[:, :1], want_var=True)
    # no training set, and a training set without a kernel id
    fresh = _lib.Device(dev.device)
    try:
        rc = fresh._lib.gpry_predict_thetas_var(fresh._h, vp(Tc), 3, vp(X), 2, vp(mean), vp(var), None, None, None)
        assert rc == -1 and "train" in fresh._lib.gpry_last_error(fresh._h).decode()
        fresh.set_train(X_, y_, a)
        rc = fresh._lib.gpry_predict_thetas_var(fresh._h, vp(Tc), 3, vp(X), 2, vp(mean), vp(var), None, None, None)
        assert rc == -1 and "kernel id" in fresh._lib.gpry_last_error(fresh._h).decode()
    finally:
        fresh.close()
    assert same_bits(dev.predict_thetas(T, Xq, want_var=True), answer)


# ------------------------------------------------------------------------------------ the regressor
def test_hyper_predict_end_to_end_on_a_fitted_regressor():
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.mc import hyper_laplace, hyper_predict, hyper_spread
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    N, d = 60, 2
    b = np.array([[0.0, 1.0]] * d)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(6.0 * X.mean(1)) + 0.1 * rng.standard_normal(N)
    kernel = Ck(1.0, [1e-3, 1e4]) * RBF([1.0] * d, [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=2, noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=7)
    gpr.append_to_data(X, y, fit_gpr=True)
    p = d + 2
    Xs = rng.uniform(0, 1, (40, d))
    ys, ss = gpr.predict(Xs, return_std=True)
    theta0, lml0 = gpr.kernel_.theta.copy(), gpr.log_marginal_likelihood_value_
    lap = hyper_laplace(gpr)
    if not lap.negdef or not lap.free.all():
        lap = lap._replace(negdef=True, free=np.ones(p, dtype=bool), cov=0.01 * np.eye(p))
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    r = hyper_predict(gpr, Xs, n_draws=16, seed=5, laplace=lap)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 17 * 40, l0 + 17)
    print(r, f"max sigma_theta / sigma_gp {np.max(r.sigma_theta / r.sigma_gp):.3f}")
    assert not r.failed.any() and r.device_ms > 0 and np.isfinite(r.sigma_total).all()
    # sigma0 against the model's own predict(return_std=True), to the bound of the closed-form test
    kid, th_full = gpr.kernel_.device_spec(d)
    th_full = np.asarray(th_full, dtype=float)
    x_lo, x_span, y_mean, y_std = gpr._affine_args()[:4]
    Xu = Xs if x_lo is None else (Xs - np.asarray(x_lo)) / np.asarray(x_span)
    X_, al = np.asarray(gpr.X_train_, dtype=float), np.broadcast_to(np.asarray(gpr.alpha, dtype=float), (N,))
    va = vm.var_numpy(X_, al, th_full, kid & ~tm.W_FLAG, True, Xu, y_std)
    vb = vm.var_via_V(X_, al, th_full, kid & ~tm.W_FLAG, True, Xu, y_std)
    bound = max(10.0 * np.max(np.abs(va - vb)), 2.0 * np.max(np.abs(ss * ss - np.maximum(va, 0.0))))
    dev0 = np.max(np.abs(r.sigma0 ** 2 - ss * ss))
    print(f"hyper_predict end to end: |sigma0^2 - std^2| {dev0:.3e}, |var0 - var_a| {np.max(np.abs(r.sigma0 ** 2 - np.maximum(va, 0))):.3e}, bound {bound:.3e}")
    # (|var0 - std^2| <= |var0 - var_a| + |var_a - std^2| <= bound + bound / 2)
    assert np.max(np.abs(r.sigma0 ** 2 - np.maximum(va, 0.0))) <= bound and dev0 <= 1.5 * bound
    assert np.all(r.sigma_total >= r.sigma_gp) and np.all(r.sigma_theta > 0)
    # the draws and their means are hyper_spread's
    spread = hyper_spread(gpr, Xs, ys, None, n_draws=16, seed=5, laplace=lap, exact=True)
    assert np.array_equal(r.dtheta, spread.dtheta) and np.array_equal(r.lml, spread.lml)
    assert np.allclose(r.sigma_theta, spread.sigma_theta_draws, rtol=1e-10, atol=0)
    mean, std, lml, info = gpr.predict_thetas(Xs, np.vstack([lap.theta, lap.theta + r.dtheta]), full=True, return_std=True)
    assert np.array_equal(mean[1:], r.means) and np.array_equal(mean[0], r.mean0) and np.array_equal(std[0], r.sigma0)
    assert np.array_equal(std[1:], np.sqrt(np.maximum(r.vars, 0.0))) and np.array_equal(lml[1:], r.lml) and not info.any()
    # nothing of the fitted model moved
    after = gpr.predict(Xs, return_std=True)
    assert np.array_equal(after[0], ys) and np.array_equal(after[1], ss) and np.array_equal(gpr.kernel_.theta, theta0)
    assert gpr.log_marginal_likelihood_value_ == lml0
