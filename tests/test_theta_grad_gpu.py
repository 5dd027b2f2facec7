"""``gpry_mean_theta_grad`` on the device: the derivative of the posterior mean in theta against the numpy closed form
(tests/tools/theta_grad_model.py, formulation (b); per column of G the allowed deviation is ten times the disagreement of the
two numpy formulations, but not below 1e-7 of the column's largest entry), y with ``gpry_predict``'s one-point bits under
clip and gates, the bits contract (alone, in a batch, at any position, in split calls, on a second context), central
differences through the device's own ``set_theta`` + ``factorize`` + ``predict``, the state contract, the refusals, and
``hyper_spread`` end to end on a fitted regressor.

Shapes, the smallest at which each piece can go wrong: (50, 1), (130, 2), (333, 5) x the four kernels x white off / on;
(300, 17) the second coordinate block; (256, 32) largest d, no padding; (1100, 8) a slice with a remainder; (2500, 4) two
slices of the one-point path.  26 points per case: 8 training rows (rows 0 and 1 are duplicates: the r = 0 branch), 16
uniform, 2 far outside where k underflows.  The x-affine is on in every second case.

Measured on an MI355X (deviation / bound of the worst column; profiles/mean_theta_grad.md): against the closed form 0.144
at worst (n130_d2_k1, the log C column: 1.4e-8 of the column's largest entry where the two numpy formulations differ by
5.9e-9), 0.072 on n333_d5_k1, 0.064 on n2500_d4_k1, at most 0.008 on the models with a white term; against the device's own
central differences 0.284 at worst (n130_d2_k0), 0.06 to 0.22 on the others.

A model of more than 32 dimensions cannot be put on a context (gpry_set_train refuses it), so the call's own d > 32 refusal
cannot be reached through the C ABI: the test pins that refusal of gpry_set_train and that the context keeps its model.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
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


@pytest.mark.parametrize("case", tm.CASES, ids=tm.IDS)
def test_gradient_against_the_closed_form_per_column(dev, case):
    tm.check_closed_form(dev, case, tm.IDS[tm.CASES.index(case)])


CLIP_CASES = [(50, 1, 1, False), (333, 5, 3, True), (300, 17, 2, True), (2500, 4, 1, False)]


@pytest.mark.parametrize("case", CLIP_CASES)
def test_value_has_the_bits_of_predict_and_clip_and_gates_leave_the_gradient_alone(dev, case):
    tm.check_value_clip_gates(dev, case)


@pytest.mark.parametrize("case", [(50, 1, 2, False), (333, 5, 3, True), (300, 17, 2, True), (1100, 8, 3, True), (2500, 4, 1, False)])
def test_same_bits_alone_in_a_batch_at_any_position_split_and_on_a_second_context(dev, other, case):
    tm.check_same_bits(dev, case, other)


@pytest.mark.parametrize("case", [(130, 2, kid, white) for kid in range(4) for white in (False, True)]
                         + [(333, 5, 0, False), (333, 5, 1, True), (333, 5, 2, False), (333, 5, 3, True)])
def test_against_central_differences_through_the_device_itself(dev, case):
    tm.check_against_own_differences(dev, case)


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
    Xq = tm.to_raw(case, rng.uniform(0, 1, (40, d)))
    pool = tm.to_raw(case, rng.uniform(0, 1, (777, d)))
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
            ("predict_grad_batch", lambda: dev.predict_grad_batch(Xq[:9], want_kinv=True)), ("sweep", sweep),
            ("predict_1", lambda: dev.predict(Xq[:1]))]


@pytest.mark.parametrize("case", [(333, 5, 3, True), (1100, 8, 2, False)])
def test_no_other_entry_point_notices_the_call_and_the_call_notices_none_of_them(dev, other, case):
    N, d, kid, white = case
    X_, y_, a, th = tm.load(other, case)
    Xq = tm.to_raw(case, tm.points(case, X_))
    fresh = other.mean_theta_grad(Xq)
    tm.load(dev, case)
    ops = others(dev, case, th)
    before = [f() for _, f in ops]
    got = dev.mean_theta_grad(Xq)
    assert same_bits(got, fresh)
    after = [f() for _, f in ops]
    for (name, _), x, y in zip(ops, before, after):
        assert same_bits(x, y), name
    for name, f in ops:
        f()
        assert same_bits(dev.mean_theta_grad(Xq), fresh), name
    # another theta: that model's fresh-context answer
    there = th.copy()
    there[:d + 1] -= 0.15
    tm.load(other, case, theta=there)
    want = other.mean_theta_grad(Xq)
    dev.lml(th, True)                                   # (the factor cache of gpry_lml holds the OLD theta's factor)
    tm.load(dev, case, theta=there)
    got = dev.mean_theta_grad(Xq)
    assert same_bits(got, want) and not np.array_equal(got["G"], fresh["G"])


def test_after_append_rows_it_agrees_with_a_fresh_factor_of_the_grown_set(dev, other):
    case = (333, 5, 3, True)
    N, d, kid, white = case
    X_, y_, a, th = tm.problem(N, d, seed=N + d, white=white)
    lo, span = tm.affine(case)
    dev.set_train(X_[:N - 3], y_[:N - 3], a[:N - 3])
    dev.set_theta(kid | tm.W_FLAG, th)
    dev.set_affine(lo, span, tm.Y_MEAN, tm.Y_STD)
    assert dev.factorize() == 0
    dev.mean_theta_grad(tm.to_raw(case, X_[:4]))        # (a call on the smaller model first: nothing of it may stay)
    assert dev.append_rows(X_[N - 3:], y_[N - 3:], a[N - 3:]) == 0
    Xq_, Ga, Gb = tm.reference(case)
    G = dev.mean_theta_grad(tm.to_raw(case, Xq_))["G"]
    tm.load(other, case)
    Gf = other.mean_theta_grad(tm.to_raw(case, Xq_))["G"]
    bound = tm.column_bound(Ga, Gb)
    print(f"append_rows: worst column ratio to the fresh factor {np.max(tm.column_dev(G, Gf) / bound):.3f}, to the closed form "
          f"{np.max(tm.column_dev(G, Gb) / bound):.3f}")
    assert np.all(tm.column_dev(G, Gf) <= bound) and np.all(tm.column_dev(G, Gb) <= bound)


# ------------------------------------------------------------------------------------ refusals
def test_refusals_return_minus_one_with_a_message_and_the_next_call_answers_as_before(dev):
    from gpry_amd import _lib
    case = (130, 2, 1, True)
    tm.load(dev, case)
    Xq = tm.to_raw(case, tm.reference(case)[0])
    good = dev.mean_theta_grad(Xq)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    X = np.ascontiguousarray(Xq[:2])
    y, G = np.empty(2), np.empty((2, 4))
    bad = X.copy()
    bad[1, 0] = np.inf
    nan = X.copy()
    nan[0, 1] = np.nan
    for what, args, word in [("NULL X", (None, 2, vp(y), vp(G)), "NULL"), ("NULL G", (vp(X), 2, vp(y), None), "NULL"),
                             ("npts 0", (vp(X), 0, vp(y), vp(G)), "npts"), ("npts < 0", (vp(X), -3, vp(y), vp(G)), "npts"),
                             ("inf", (vp(bad), 2, vp(y), vp(G)), "not finite"), ("nan", (vp(nan), 2, vp(y), vp(G)), "not finite")]:
        rc = dev._lib.gpry_mean_theta_grad(dev._h, *args, None)
        msg = dev._lib.gpry_last_error(dev._h).decode()
        assert rc == -1 and word in msg and "gpry_mean_theta_grad" in msg, (what, rc, msg)
        assert same_bits(dev.mean_theta_grad(Xq), good), what
    # y_out is optional
    assert dev._lib.gpry_mean_theta_grad(dev._h, vp(X), 2, None, vp(G), None) == 0
    assert np.array_equal(G, good["G"][:2])
    # no valid factor: a theta without a factorisation
    N, d, kid, white = case
    dev.set_theta(kid | tm.W_FLAG, tm.problem(N, d, seed=N + d, white=white)[3] + 0.05)
    with pytest.raises(_lib.GpryHipError, match="factor"):
        dev.mean_theta_grad(Xq)
    tm.load(dev, case)
    assert same_bits(dev.mean_theta_grad(Xq), good)
    # no model at all
    fresh = _lib.Device(dev.device)
    fresh.d = 2
    try:
        with pytest.raises(_lib.GpryHipError, match="gpry_mean_theta_grad|train"):
            fresh.mean_theta_grad(X)
    finally:
        fresh.close()
    # d > 32: such a model never reaches the call -- gpry_set_train refuses it, naming the limit, and the context keeps
    # the model it had (the call's own d > 32 refusal stands behind that one)
    X33 = np.random.default_rng(0).uniform(0, 1, (40, 33))
    with pytest.raises(_lib.GpryHipError, match="32"):
        dev.set_train(X33, np.sin(X33.sum(1)), np.full(40, 1e-4))
    tm.load(dev, case)
    assert same_bits(dev.mean_theta_grad(Xq), good)


def test_stage_timers_and_more_points_than_one_chunk(dev):
    case = (50, 1, 0, False)
    assert tm.affine(case)[0] is None                   # (raw coordinates are the unit ones)
    X_, y_, a, th = tm.load(dev, case)
    rng = np.random.default_rng(5)
    Xq = rng.uniform(0, 1, (65536 + 300, 1))
    dev.timing_reset()
    out = dev.mean_theta_grad(Xq)
    assert dev.timing("theta_grad_setup")[1] == 1 and dev.timing("theta_grad")[1] == 2 and out["device_ms"] > 0
    pick = np.array([0, 65535, 65536, len(Xq) - 1])
    few = dev.mean_theta_grad(Xq[pick])
    assert np.array_equal(out["G"][pick], few["G"]) and np.array_equal(out["y"][pick], few["y"])
    Ga = tm.grad_explicit(X_, y_, a, th, 0, False, Xq[pick], tm.Y_STD)
    Gb = tm.grad_via_V(X_, y_, a, th, 0, False, Xq[pick], tm.Y_STD)
    assert np.all(tm.column_dev(few["G"], Gb) <= tm.column_bound(Ga, Gb))


# ------------------------------------------------------------------------------------ the regressor
def test_hyper_spread_end_to_end_on_a_fitted_regressor():
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.mc import hyper_laplace, hyper_spread
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    N, d = 60, 2
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
    Xs = rng.uniform(0, 1, (500, d))
    ys = gpr.predict(Xs)
    w = rng.uniform(0.5, 1.5, 500)
    w[:7] = 0.0
    n0 = gpr.n_eval
    mean, G = gpr.mean_theta_grad(Xs, full=True)
    assert gpr.n_eval == n0 + 500 and G.shape == (500, 4) and np.isfinite(G).all()
    assert np.array_equal(mean[:20], np.array([gpr.predict(x[None, :])[0] for x in Xs[:20]]))
    assert np.array_equal(gpr.mean_theta_grad(Xs)[1], G)            # theta is the device's own vector here
    lap = hyper_laplace(gpr)
    print(f"hyper_laplace: free {lap.free}, negdef {lap.negdef}, sigma_log {lap.sigma_log}")
    if not lap.negdef or not lap.free.any():
        with pytest.raises(ValueError):
            hyper_spread(gpr, Xs, ys, w, laplace=lap)
        lap = lap._replace(negdef=True, free=np.ones(4, dtype=bool), cov=0.01 * np.eye(4))
    r = hyper_spread(gpr, Xs, ys, w, n_draws=64, seed=5, laplace=lap)
    print(r)
    keep = np.flatnonzero(w > 0)
    assert np.array_equal(r.keep, keep) and r.n_points == 493 and r.dtheta.shape == (64, 4) and r.device_ms > 0
    assert np.all(r.dtheta[:, ~lap.free] == 0.0)
    wk = w[keep] / w[keep].sum()
    Gk = G[keep]
    logr = r.dtheta.dot(Gk.T)
    ws = wk * np.exp(logr)
    dlogZ = np.log(ws.sum(axis=1))
    ws /= ws.sum(axis=1)[:, None]
    means = ws.dot(Xs[keep])
    cen = Xs[keep][None, :, :] - means[:, None, :]
    covs = np.einsum("si,sia,sib->sab", ws, cen, cen)
    assert np.allclose(r.dlogZ, dlogZ, rtol=0, atol=1e-12) and np.allclose(r.means, means, rtol=0, atol=1e-13)
    # (sums of 493 terms below 1 in float64, formed in two orders: 493 x 1.1e-16 = 5e-14)
    assert np.allclose(r.covs, covs, rtol=0, atol=1e-13) and np.allclose(r.ess, 1.0 / np.sum(ws * ws, axis=1), rtol=1e-12)
    Gf = Gk[:, lap.free]
    assert np.allclose(r.sigma_theta, np.sqrt(np.einsum("if,fg,ig->i", Gf, lap.cov, Gf)), rtol=1e-12)
    assert r.max_abs_logr == np.max(np.abs(logr)) and abs(r.logZ_std - dlogZ.std()) <= 1e-12
