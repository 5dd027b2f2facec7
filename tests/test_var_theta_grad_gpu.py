"""``gpry_var_theta_grad`` on the device: the derivative of the latent predictive variance in theta against the numpy closed
form (tests/tools/var_theta_grad_model.py, formulation (b); per column of G the allowed deviation is ten times the
disagreement of the two numpy formulations, but not below 1e-7 of the column's largest entry), var against the refactorised
closed form, the bits contract (alone, in a batch, at any position, in split calls, across panels and chunks, on a second
context), central differences through the device's own ``predict_thetas(.., want_var=True)``, ``append_rows``, the state
contract, the refusals, and ``hyper_acq_spread`` end to end on a fitted regressor.

Shapes, the smallest at which each piece can go wrong (``theta_grad_model.CASES``): (50, 1), (130, 2), (333, 5) x the four
kernels x white off / on -- padding below and across 128 rows; (300, 17) the second coordinate block; (256, 32) largest d, no
padding; (1100, 8) a slice with a remainder; (2500, 4) several row tiles.  26 points per case: 8 training rows (rows 0 and 1
are duplicates: the r = 0 branch), 16 uniform, 2 far outside where k underflows and the row is exactly
[y_std^2 C, 0 .., y_std^2 w].  The x-affine is on in every second case.

Measured on an MI355X (deviation / bound; profiles/var_theta_grad.md): G against the closed form 9.7e-4 at worst (n50_d1_k0,
the log l column: 9.7e-11 of the column's largest entry where the two numpy formulations differ by 1.5e-9 and the floor of
1e-7 decides the bound), below 1e-4 on every other case; var 0.46 at worst (n256_d32_k0: 7.1e-15 against a bound of 1.5e-14,
twice what ``predict_thetas_var`` deviates by; 0.44 on n50_d1_k0_w), 0.06 to 0.29 on the others; against the device's own central differences 0.39
at worst (n130_d2_k0), 0.02 to 0.16 on the others.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import var_theta_grad_model as vm  # noqa: E402

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


@pytest.mark.parametrize("case", vm.CASES, ids=vm.IDS)
def test_gradient_against_the_closed_form_per_column(dev, case):
    vm.check_closed_form(dev, case, vm.IDS[vm.CASES.index(case)])


@pytest.mark.parametrize("case", vm.CASES, ids=vm.IDS)
def test_variance_against_the_refactorised_closed_form(dev, case):
    vm.check_var(dev, case, vm.IDS[vm.CASES.index(case)])


@pytest.mark.parametrize("case", [(50, 1, 2, False), (333, 5, 3, True), (300, 17, 2, True), (1100, 8, 3, True), (2500, 4, 1, False)])
def test_same_bits_alone_in_a_batch_at_any_position_split_and_on_a_second_context(dev, other, case):
    vm.check_same_bits(dev, case, other)


def test_more_points_than_one_panel_and_than_one_chunk(dev):
    case = (130, 2, 1, False)
    X_, y_, a, th = vm.load(dev, case)
    pc = dev.var_theta_grad_panel()                     # (of this model: a function of its padded size)
    assert pc >= 64 and pc % 64 == 0
    rng = np.random.default_rng(5)

    def spot(n, edges):
        Xq = vm.to_raw(case, rng.uniform(0, 1, (n, 2)))
        out = dev.var_theta_grad(Xq)
        pick = np.unique(np.concatenate([[0, n - 1]] + [[e - 1, e] for e in edges]))
        few = dev.var_theta_grad(Xq[pick])
        assert np.array_equal(out["G"][pick], few["G"]) and np.array_equal(out["var"][pick], few["var"])
        for i in pick[:3]:
            one = dev.var_theta_grad(Xq[i:i + 1])
            assert np.array_equal(one["G"][0], out["G"][i]) and one["var"][0] == out["var"][i]
        return Xq[pick], few

    dev.timing_reset()
    Xp, few = spot(3 * pc + 5, [pc, 2 * pc, 3 * pc])
    # (the whole batch: four panels; the picked rows and three single rows: one panel each)
    assert dev.timing("var_theta_grad_setup")[1] == 5 and dev.timing("var_theta_grad")[1] == 8
    for stage in ("var_theta_grad_panel", "var_theta_grad_solve", "var_theta_grad_products", "var_theta_grad_finish"):
        assert dev.timing(stage)[1] == 8, stage
    assert vm.affine(case)[0] is None                   # (raw coordinates are the unit ones)
    Xp_ = Xp
    _, Ga = vm.grad_explicit(X_, a, th, 1, False, Xp_, vm.Y_STD)
    _, Gb = vm.grad_via_V(X_, a, th, 1, False, Xp_, vm.Y_STD)
    assert np.all(vm.column_dev(few["G"], Gb) <= vm.column_bound(Ga, Gb))
    spot(65536 + 5, [65536])


@pytest.mark.parametrize("case", [(130, 2, kid, white) for kid in range(4) for white in (False, True)]
                         + [(333, 5, 0, False), (333, 5, 1, True), (333, 5, 2, False), (333, 5, 3, True)])
def test_against_central_differences_through_the_device_s_own_variance(dev, case):
    vm.check_against_own_differences(dev, case)


def test_after_append_rows_it_agrees_with_a_fresh_factor_of_the_grown_set(dev, other):
    case = (333, 5, 3, True)
    N, d, kid, white = case
    X_, y_, a, th = vm.problem(N, d, seed=N + d, white=white)
    lo, span = vm.affine(case)
    dev.set_train(X_[:N - 16], y_[:N - 16], a[:N - 16])
    dev.set_theta(kid | vm.W_FLAG, th)
    dev.set_affine(lo, span, vm.Y_MEAN, vm.Y_STD)
    assert dev.factorize() == 0
    dev.var_theta_grad(vm.to_raw(case, X_[:4]))         # (a call on the smaller model first: nothing of it may stay)
    assert dev.append_rows(X_[N - 16:], y_[N - 16:], a[N - 16:]) == 0
    Xq_, Ga, Gb, va, vb = vm.reference(case)
    out = dev.var_theta_grad(vm.to_raw(case, Xq_))
    vm.load(other, case)
    fresh = other.var_theta_grad(vm.to_raw(case, Xq_))
    bound = vm.column_bound(Ga, Gb)
    print(f"append_rows: worst column ratio to the fresh factor {np.max(vm.column_dev(out['G'], fresh['G']) / bound):.3f}, to the "
          f"closed form {np.max(vm.column_dev(out['G'], Gb) / bound):.3f}")
    assert np.all(vm.column_dev(out["G"], fresh["G"]) <= bound) and np.all(vm.column_dev(out["G"], Gb) <= bound)
    assert np.max(np.abs(out["var"] - fresh["var"])) <= 1e-9 * np.max(va)


# ------------------------------------------------------------------------------------ state
def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a if k != "device_ms")
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def others(dev, case, th):
    """The other entry points, one call each: name -> answer."""
    N, d, kid, white = case
    rng = np.random.default_rng(3)
    Xq = vm.to_raw(case, rng.uniform(0, 1, (40, d)))
    pool = vm.to_raw(case, rng.uniform(0, 1, (777, d)))
    alt = th.copy()
    alt[:d + 1] += 0.1

    def sweep():
        out = dev.sweep_logexp(pool, 1.0, 0.0, 0.0)
        top, bound = dev.sweep_topk(5)
        return [out["y"], out["sigma"], out["acq"], top["idx"], top["acq"], bound]

    def loo():
        r = dev.loo()
        return [r[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")]

    return [("predict_std", lambda: dev.predict(Xq, return_std=True)), ("lml_grad", lambda: dev.lml(alt, True)), ("loo", loo),
            ("sweep", sweep), ("predict_1", lambda: dev.predict(Xq[:1])), ("mean_theta_grad", lambda: dev.mean_theta_grad(Xq)),
            ("predict_without", lambda: dev.predict_without([[0, 5, 7], [N - 1]], Xq)),
            ("lml_hessian", lambda: dev.lml_hessian(alt))]


@pytest.mark.parametrize("case", [(333, 5, 3, True), (1100, 8, 2, False)])
def test_no_other_entry_point_notices_the_call_and_the_call_notices_none_of_them(dev, other, case):
    N, d, kid, white = case
    X_, y_, a, th = vm.load(other, case)
    Xq = vm.to_raw(case, vm.points(case, X_))
    fresh = other.var_theta_grad(Xq)
    vm.load(dev, case)
    ops = others(dev, case, th)
    before = [f() for _, f in ops]
    got = dev.var_theta_grad(Xq)
    assert same_bits(got, fresh)
    after = [f() for _, f in ops]
    for (name, _), x, y in zip(ops, before, after):
        assert same_bits(x, y), name
    for name, f in ops:
        f()
        assert same_bits(dev.var_theta_grad(Xq), fresh), name
    # another theta: that model's fresh-context answer
    there = th.copy()
    there[:d + 1] -= 0.15
    vm.load(other, case, theta=there)
    want = other.var_theta_grad(Xq)
    dev.lml(th, True)                                   # (the factor cache of gpry_lml holds the OLD theta's factor)
    vm.load(dev, case, theta=there)
    got = dev.var_theta_grad(Xq)
    assert same_bits(got, want) and not np.array_equal(got["G"], fresh["G"])
    # the stage timers exist
    dev.timing_reset()
    out = dev.var_theta_grad(Xq)
    assert dev.timing("var_theta_grad_setup")[1] == 1 and dev.timing("var_theta_grad")[1] == 1 and out["device_ms"] > 0


# ------------------------------------------------------------------------------------ refusals
def test_refusals_return_minus_one_with_a_message_and_the_next_call_answers_as_before(dev):
    from gpry_amd import _lib
    case = (130, 2, 1, True)
    vm.load(dev, case)
    Xq = vm.to_raw(case, vm.reference(case)[0])
    good = dev.var_theta_grad(Xq)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    X = np.ascontiguousarray(Xq[:2])
    v, G = np.empty(2), np.empty((2, 4))
    bad = X.copy()
    bad[1, 0] = np.inf
    nan = X.copy()
    nan[0, 1] = np.nan
    for what, args, word in [("NULL X", (None, 2, vp(v), vp(G)), "NULL"), ("NULL G", (vp(X), 2, vp(v), None), "NULL"),
                             ("npts 0", (vp(X), 0, vp(v), vp(G)), "npts"), ("npts < 0", (vp(X), -3, vp(v), vp(G)), "npts"),
                             ("inf", (vp(bad), 2, vp(v), vp(G)), "not finite"), ("nan", (vp(nan), 2, vp(v), vp(G)), "not finite")]:
        rc = dev._lib.gpry_var_theta_grad(dev._h, *args, None)
        msg = dev._lib.gpry_last_error(dev._h).decode()
        assert rc == -1 and word in msg and "gpry_var_theta_grad" in msg, (what, rc, msg)
        assert same_bits(dev.var_theta_grad(Xq), good), what
    # var_out is optional
    assert dev._lib.gpry_var_theta_grad(dev._h, vp(X), 2, None, vp(G), None) == 0
    assert np.array_equal(G, good["G"][:2])
    assert dev.var_theta_grad(X, want_var=False)["var"] is None
    # a wrong width never reaches the library
    with pytest.raises(ValueError, match="shape"):
        dev.var_theta_grad(np.zeros((3, 5)))
    # no valid factor: a theta without a factorisation
    N, d, kid, white = case
    dev.set_theta(kid | vm.W_FLAG, vm.problem(N, d, seed=N + d, white=white)[3] + 0.05)
    with pytest.raises(_lib.GpryHipError, match="factor"):
        dev.var_theta_grad(Xq)
    vm.load(dev, case)
    assert same_bits(dev.var_theta_grad(Xq), good)
    # no model at all
    fresh = _lib.Device(dev.device)
    fresh.d = 2
    try:
        with pytest.raises(_lib.GpryHipError, match="gpry_var_theta_grad"):
            fresh.var_theta_grad(X)
    finally:
        fresh.close()


def test_a_model_above_4096_padded_rows_is_refused_before_anything_is_launched(dev):
    from gpry_amd._lib import GpryHipError
    N = 4097
    rng = np.random.default_rng(1)
    X_ = rng.uniform(0, 1, (N, 1))
    dev.set_train(X_, np.sin(3 * X_[:, 0]), np.full(N, 1e-4))
    dev.set_theta(0, np.log([2.0, 0.3]))
    dev.set_affine(None, None, 0.0, 1.0)
    assert dev.factorize() == 0
    dev.timing_reset()
    with pytest.raises(GpryHipError, match="4096"):
        dev.var_theta_grad(X_[:3])
    for stage in ("var_theta_grad_setup", "var_theta_grad", "var_theta_grad_panel", "var_theta_grad_products"):
        assert dev.timing(stage)[1] == 0, stage
    # the context answers the next call as before
    case = (130, 2, 1, True)
    vm.check_closed_form(dev, case)


# ------------------------------------------------------------------------------------ the regressor
def test_hyper_acq_spread_end_to_end_on_a_fitted_regressor():
    from gpry_amd.acquisition_functions import LogExp
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.hyper import acq_spread_fields
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.mc import hyper_acq_spread, hyper_laplace
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    N, d = 120, 3
    b = np.array([[0.0, 1.0]] * d)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(N)
    kernel = Ck(1.0, [1e-3, 1e4]) * RBF([1.0] * d, [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=3, noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=7)
    gpr.append_to_data(X, y, fit_gpr=True)
    gpr.fit_gpr_hyperparameters()
    Xs = np.vstack([rng.uniform(0, 1, (40, d)), X[:3]])
    n0 = gpr.n_eval
    var, G = gpr.var_theta_grad(Xs, full=True)
    assert gpr.n_eval == n0 + 43 and G.shape == (43, 5) and np.isfinite(G).all() and np.all(var > 0)
    assert np.array_equal(gpr.var_theta_grad(Xs)[1], G)             # theta is the device's own vector here
    # the variance is the one predict_thetas reports at the fitted theta, to the rounding of two summation orders
    std = gpr.predict_thetas(Xs, gpr.kernel_.theta[None, :], return_std=True)[1][0]
    assert np.allclose(np.sqrt(var), std, rtol=1e-6)
    lap = hyper_laplace(gpr)
    print(f"hyper_laplace: free {lap.free}, negdef {lap.negdef}, sigma_log {lap.sigma_log}")
    if not lap.negdef or not lap.free.any():
        with pytest.raises(ValueError):
            hyper_acq_spread(gpr, Xs, laplace=lap)
        lap = lap._replace(negdef=True, free=np.ones(5, dtype=bool), cov=0.01 * np.eye(5))
    acq = LogExp(zeta=0.4, sigma_n=float(np.sqrt(np.sort(var)[1:3].mean())))        # two dead rows
    r = hyper_acq_spread(gpr, Xs, acq=acq, laplace=lap)
    print(r)
    mean, Gm = gpr.mean_theta_grad(Xs, full=True)
    assert np.array_equal(r.mean, mean) and np.array_equal(r.var, var) and np.array_equal(r.G_mean, Gm)
    assert np.array_equal(r.G_var, G) and r.device_ms > 0 and r.baseline == gpr.y_max
    f = acq_spread_fields(mean, var, Gm, G, lap.cov, lap.free, 0.4, acq.sigma_n, gpr.y_max)
    for name, val in f.items():
        assert np.array_equal(getattr(r, name), val, equal_nan=True), name
    dead = np.isneginf(r.acq)
    assert dead.sum() == 2 and np.all(np.isnan(r.acq_grad[dead])) and np.all(np.isnan(r.top_flip[dead]))
    live = np.flatnonzero(~dead)
    ex = var[live] - acq.sigma_n ** 2
    assert np.allclose(r.acq[live], 0.8 * (mean[live] - gpr.y_max) + 0.5 * np.log(ex), rtol=0, atol=1e-13)
    assert np.allclose(r.acq_grad[live], 0.8 * Gm[live] + G[live] / (2 * ex)[:, None], rtol=1e-13)
    Af = r.acq_grad[live][:, lap.free]
    assert np.allclose(r.acq_sigma_theta[live], np.sqrt(np.einsum("if,fg,ig->i", Af, lap.cov, Af)), rtol=1e-12)
    assert np.all(np.diff(r.acq[r.order][:len(live)]) <= 0) and np.all(dead[r.order[len(live):]])
    assert sorted(r.order) == list(range(43))
    fl = r.flip[np.ix_(live, live)]
    assert np.array_equal(fl, fl.T) and np.all(np.diag(fl) == 0.5) and np.all((fl >= 0) & (fl <= 0.5))
    assert r.top_flip[r.order[0]] == 0.0 and np.allclose(np.delete(r.top_flip[live], np.flatnonzero(live == r.order[0])),
                                                           np.delete(r.flip[live, r.order[0]], np.flatnonzero(live == r.order[0])))
