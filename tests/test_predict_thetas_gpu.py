"""``gpry_predict_thetas`` on the device: the posterior mean at M points under B thetas in one call, against the numpy truth
(tests/tools/predict_thetas_model.py), the bits contract, a theta that is not positive definite among good ones, the state
contract, the refusals, and ``hyper_spread(exact=True)`` end to end on a fitted regressor.

Shapes, the smallest at which each piece can go wrong: (50, 1) Np = 128, the one-after-another route; (130, 2) x the four
kernels x white off / on, the smallest batched size (Np = 256); (333, 5) a padded remainder; (300, 17) the second coordinate
block; (256, 32) largest d, no padding; (1100, 8) several panel steps; (2500, 4) the largest.  Thetas per case: the model's
theta as row 0 and 4 rows at theta + 0.3 N(0, 1) from a fixed seed.  26 points per case: 8 training rows (rows 0 and 1 are
duplicates), 16 uniform, 2 far outside where k underflows and the mean is y_mean exactly.  The x-affine is on in every
second case of tests/tools/theta_grad_model.py's list.

The bound against the closed form, per theta row: max_i |mean_dev - mean_a| <= max(10 max_i |mean_a - mean_b|, 2 D_seq),
mean_a / mean_b the two numpy formulations (triangular solves / explicit V = L^-1) and D_seq the deviation from (a) of the
route that exists without this call -- set_theta + factorize + predict with clip off and no gates -- on the same device in
the same test.  The first term is test_lml_hessian_gpu.py's rule; the second measures the call against other code, with a
factor 2 because both routes add the same N terms in different orders: errors of one size, independent, no room for a lost
digit.

The call evaluates a point with the arithmetic of gpry_predict's one-point path (csrc/predict_thetas.hip), so beside the
bound the test asserts that every row equals ``predict(x[None])`` at that theta bit for bit (clip off, no gates).

Measured on an MI355X (deviation / bound of the worst theta row; profiles/predict_thetas.md): n50_d1_k1 0.187; n130_d2 k0
0.242, k0_w 0.143, k1 0.190, k1_w 0.169, k2 0.229, k2_w 0.181, k3 0.489, k3_w 0.161; n333_d5_k2_w 0.334; 0.500 on
n300_d17_k2_w, n256_d32_k0, n1100_d8_k3_w and n2500_d4_k1, where the second term of the bound decides and the call has the
bits of the sequential route's 26-point predict as well.  The deviations are 1e-14 to 1.2e-11 of max|mean - y_mean|.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict_thetas_model as pm  # noqa: E402
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


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("mean", "lml", "info"))


# ------------------------------------------------------------------------------------ against the closed form
@pytest.mark.parametrize("case", pm.CASES, ids=pm.IDS)
def test_mean_against_the_closed_form_and_lml_with_the_bits_of_lml(dev, case):
    N, d, kid, white = case
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    out = dev.predict_thetas(T, Xq)
    assert out["mean"].shape == (5, len(Xq)) and out["lml"].shape == (5,) and out["info"].shape == (5,)
    assert np.isfinite(out["mean"]).all() and not out["info"].any() and out["device_ms"] > 0
    # lml and info: gpry_lml's, bit for bit
    for b in range(5):
        val, info = dev.lml(T[b], False)
        assert out["lml"][b] == val and out["info"][b] == info, (b, out["lml"][b], val)
    # far outside k underflows: y_mean exactly
    assert np.all(out["mean"][:, -2:] == tm.Y_MEAN)
    worst = 0.0
    try:
        for b in range(5):
            ma = tm.mean_numpy(X_, y_, a, T[b], kid, white, Xq_, tm.Y_MEAN, tm.Y_STD)
            mb = pm.mean_via_V(X_, y_, a, T[b], kid, white, Xq_, tm.Y_MEAN, tm.Y_STD)
            dev.set_theta(flag(case), T[b])
            assert dev.factorize() == 0
            seq = dev.predict(Xq)
            # the call's arithmetic is the one-point path's: its bits at this theta, clip off and no gates
            assert np.array_equal(out["mean"][b], np.array([dev.predict(x[None, :])[0] for x in Xq])), b
            ab, d_seq, d_dev = np.max(np.abs(ma - mb)), np.max(np.abs(seq - ma)), np.max(np.abs(out["mean"][b] - ma))
            bound = max(10.0 * ab, 2.0 * d_seq)
            scale = np.max(np.abs(ma - tm.Y_MEAN))
            print(f"predict_thetas {pm.IDS[pm.CASES.index(case)]} row {b}: deviation {d_dev:.3e} ({d_dev / scale:.2e} of max|mean - y_mean|), "
                  f"a-b {ab:.3e}, sequential route {d_seq:.3e}, ratio {d_dev / bound:.3f}")
            worst = max(worst, d_dev / bound)
            assert d_dev <= bound, (b, d_dev, ab, d_seq)
    finally:
        tm.load(dev, case)
    print(f"predict_thetas {pm.IDS[pm.CASES.index(case)]}: worst ratio {worst:.3f}")


# ------------------------------------------------------------------------------------ bits
def two_sets_mb(dev):
    """``lml_batch_mb`` at which exactly two scratch sets of the last batched call's layout fit (test_loo_batch_gpu.py)."""
    per_set = 8 * dev.timing("batch_set_doubles")[1]
    assert per_set > 0
    mb = -(-2 * per_set // (1 << 20))
    assert (mb << 20) // per_set == 2, (mb, per_set)
    return mb


@pytest.mark.parametrize("case", [(50, 1, 1, False), (130, 2, 0, False), (130, 2, 3, True), (333, 5, 2, True), (300, 17, 2, True),
                                  (256, 32, 0, False), (1100, 8, 3, True), (2500, 4, 1, False)])
def test_same_bits_whatever_the_batch_the_position_the_chunking_the_route_and_the_context(dev, other, case):
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    whole = dev.predict_thetas(T, Xq)
    assert same(dev.predict_thetas(T, Xq), whole)                                   # a second call repeats the first
    batched = dev.N > 128
    if batched:
        assert dev.timing("batch_chunk")[1] == 5
    # a row alone, and at another position
    for b in (0, 3):
        one = dev.predict_thetas(T[b:b + 1], Xq)
        assert np.array_equal(one["mean"][0], whole["mean"][b]) and one["lml"][0] == whole["lml"][b]
    perm = np.array([4, 2, 0, 1, 3])
    moved = dev.predict_thetas(T[perm], Xq)
    assert np.array_equal(moved["mean"], whole["mean"][perm]) and np.array_equal(moved["lml"], whole["lml"][perm])
    # points permuted, and split over two calls
    pp = np.random.default_rng(1).permutation(len(Xq))
    assert np.array_equal(dev.predict_thetas(T, Xq[pp])["mean"], whole["mean"][:, pp])
    left, right = dev.predict_thetas(T, Xq[:11]), dev.predict_thetas(T, Xq[11:])
    assert np.array_equal(np.hstack([left["mean"], right["mean"]]), whole["mean"]) and np.array_equal(left["lml"], whole["lml"])
    keys = ("lml_batch_mb", "panel_debug", "lml_batch", "lml_schedule")
    keep = {k: dev.get_option(k) for k in keys}
    try:
        if batched:
            # exactly two sets fit: 2 + 2 + 1, every scratch set starting as NaNs
            dev.set_option("lml_batch_mb", two_sets_mb(dev))
            dev.set_option("panel_debug", keep["panel_debug"] | 128)
            assert same(dev.predict_thetas(T, Xq), whole)
            assert dev.timing("batch_chunk")[1] == 2
            dev.set_option("lml_batch_mb", keep["lml_batch_mb"])
            dev.set_option("panel_debug", keep["panel_debug"])
        # one after another
        dev.set_option("lml_batch", 0)
        assert same(dev.predict_thetas(T, Xq), whole)
        dev.set_option("lml_batch", keep["lml_batch"])
        # the throughput schedule of gpry_lml_batch is not this call's
        dev.set_option("lml_schedule", 1)
        assert same(dev.predict_thetas(T, Xq), whole)
    finally:
        for k in keys:
            dev.set_option(k, keep[k])
    # a second context
    tm.load(other, case)
    assert same(other.predict_thetas(T, Xq), whole)


def test_the_chunk_boundary_of_the_points(dev):
    case = (130, 2, 0, False)
    X_, y_, a, th, T, Xq_, _ = setup(dev, case)
    Xq = tm.to_raw(case, np.random.default_rng(5).uniform(0, 1, (65536 + 3, 2)))
    dev.timing_reset()
    out = dev.predict_thetas(T[:2], Xq)
    assert dev.timing("predict_thetas")[1] == 1 and dev.timing("predict_thetas_mean")[1] == 2
    cut = 40000
    left, right = dev.predict_thetas(T[:2], Xq[:cut]), dev.predict_thetas(T[:2], Xq[cut:])
    assert np.array_equal(np.hstack([left["mean"], right["mean"]]), out["mean"])
    pick = np.array([0, 65535, 65536, 65538])
    few = dev.predict_thetas(T[:2], Xq[pick])
    assert np.array_equal(few["mean"], out["mean"][:, pick])
    for b in range(2):
        ma = tm.mean_numpy(X_, y_, a, T[b], 0, False, dev_unit(case, Xq[pick]), tm.Y_MEAN, tm.Y_STD)
        # (cond(K) <= 2e6 on these models: float64 itself loses 2e6 x 1.1e-16 = 2e-10 of the mean's size; five times that)
        assert np.max(np.abs(few["mean"][b] - ma)) <= 1e-9 * np.max(np.abs(ma))


def dev_unit(case, Xq):
    lo, span = tm.affine(case)
    return Xq if lo is None else (Xq - lo) / span


# ------------------------------------------------------------------------------------ a theta that is not positive definite
@pytest.mark.parametrize("N,d,kid", [(100, 3, 0), (300, 5, 2)])
def test_a_theta_that_is_not_positive_definite_fails_on_its_own(dev, N, d, kid):
    """test_lml_batch_gpu.py's construction: six duplicated training points, which every other theta survives thanks to the
    noise on their diagonal entries; at C = 1e15 that noise is below half an ulp of the diagonal."""
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
    without = dev.predict_thetas(T[good], Xq)
    assert not without["info"].any()
    out = dev.predict_thetas(T, Xq)
    assert out["info"][bad] > 0 and np.isneginf(out["lml"][bad]) and np.isnan(out["mean"][bad]).all()
    assert (out["lml"][bad], out["info"][bad]) == dev.lml(T[bad], False)
    assert np.array_equal(out["mean"][good], without["mean"]) and np.array_equal(out["lml"][good], without["lml"])
    assert not out["info"][good].any()
    alone = dev.predict_thetas(T[bad:bad + 1], Xq)
    assert alone["info"][0] > 0 and np.isneginf(alone["lml"][0]) and np.isnan(alone["mean"]).all()


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
    """The other entry points, one call each: name -> answer (test_theta_grad_gpu.py's list, with mean_theta_grad and
    lml_hessian)."""
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
            ("predict_1", lambda: dev.predict(Xq[:1])), ("mean_theta_grad", lambda: dev.mean_theta_grad(Xq)),
            ("lml_hessian", lambda: dev.lml_hessian(alt))]


def check_state(dev, case, th, T, Xq, fresh):
    ops = others(dev, case, th)
    before = [f() for _, f in ops]
    assert same_bits(dev.predict_thetas(T, Xq), fresh)
    after = [f() for _, f in ops]
    for (name, _), x, y in zip(ops, before, after):
        assert same_bits(x, y), name
    for name, f in ops:
        f()
        assert same_bits(dev.predict_thetas(T, Xq), fresh), name


@pytest.mark.parametrize("case", [(50, 1, 1, False), (333, 5, 3, True), (1100, 8, 2, False)])
def test_no_other_entry_point_notices_the_call_and_the_call_notices_none_of_them(dev, other, case):
    X_, y_, a, th, T, Xq_, Xq = setup(other, case)
    fresh = other.predict_thetas(T, Xq)
    tm.load(dev, case)
    check_state(dev, case, th, T, Xq, fresh)
    # with gates set
    lo_hi = np.stack([Xq[:24].min(axis=0) - 1.0, Xq[:24].max(axis=0) + 1.0], axis=1)
    lo_hi[0, 1] = np.sort(Xq[:24, 0])[12]
    dev.set_gates(trust_bounds=lo_hi)
    try:
        check_state(dev, case, th, T, Xq, fresh)
    finally:
        dev.set_gates()
    # the factor cache of gpry_lml: a factor adopted after the call is the theta's own
    dev.lml(T[1], True)
    dev.predict_thetas(T, Xq)
    dev.set_theta(flag(case), T[1])
    assert dev.factorize() == 0
    got = dev.predict(Xq)
    other.set_theta(flag(case), T[1])
    assert other.factorize() == 0
    assert np.array_equal(got, other.predict(Xq))


def test_with_a_grown_factor_nothing_notices_and_the_call_sees_the_grown_set(dev, other):
    case = (333, 5, 3, True)
    N, d, kid, white = case
    X_, y_, a, th = tm.problem(N, d, seed=N + d, white=white)
    lo, span = tm.affine(case)
    dev.set_train(X_[:N - 3], y_[:N - 3], a[:N - 3])
    dev.set_theta(kid | tm.W_FLAG, th)
    dev.set_affine(lo, span, tm.Y_MEAN, tm.Y_STD)
    assert dev.factorize() == 0
    T = pm.thetas_of(case, th)
    Xq = tm.to_raw(case, tm.points(case, X_))
    dev.predict_thetas(T, Xq)                           # (a call on the smaller model first: nothing of it may stay)
    assert dev.append_rows(X_[N - 3:], y_[N - 3:], a[N - 3:]) == 0
    tm.load(other, case)
    fresh = other.predict_thetas(T, Xq)                 # the chain refactorises: the grown SET decides, not how the factor grew
    check_state(dev, case, th, T, Xq, fresh)


# ------------------------------------------------------------------------------------ refusals
def test_refusals_return_minus_one_with_a_message_and_the_context_predicts_as_before(dev):
    from gpry_amd import _lib
    case = (130, 2, 1, True)
    X_, y_, a, th, T, Xq_, Xq = setup(dev, case)
    good = dev.predict(Xq)
    answer = dev.predict_thetas(T, Xq)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    X = np.ascontiguousarray(Xq[:2])
    Tc = np.ascontiguousarray(T[:3])
    mean, lml, info = np.empty((3, 2)), np.empty(3), np.zeros(3, dtype=np.int32)
    xinf, xnan, tinf, tnan = X.copy(), X.copy(), Tc.copy(), Tc.copy()
    xinf[1, 0], xnan[0, 1], tinf[2, 1], tnan[0, 3] = np.inf, np.nan, -np.inf, np.nan
    for what, args, word in [("NULL thetas", (None, 3, vp(X), 2, vp(mean)), "NULL"), ("NULL X", (vp(Tc), 3, None, 2, vp(mean)), "NULL"),
                             ("NULL mean", (vp(Tc), 3, vp(X), 2, None), "NULL"), ("B 0", (vp(Tc), 0, vp(X), 2, vp(mean)), "B = 0"),
                             ("B < 0", (vp(Tc), -1, vp(X), 2, vp(mean)), "B = -1"), ("M 0", (vp(Tc), 3, vp(X), 0, vp(mean)), "M = 0"),
                             ("M < 0", (vp(Tc), 3, vp(X), -2, vp(mean)), "M = -2"),
                             ("x inf", (vp(Tc), 3, vp(xinf), 2, vp(mean)), "not finite"), ("x nan", (vp(Tc), 3, vp(xnan), 2, vp(mean)), "not finite"),
                             ("theta inf", (vp(tinf), 3, vp(X), 2, vp(mean)), "not finite"),
                             ("theta nan", (vp(tnan), 3, vp(X), 2, vp(mean)), "not finite")]:
        rc = dev._lib.gpry_predict_thetas(dev._h, *args, vp(lml), vp(info), None)
        msg = dev._lib.gpry_last_error(dev._h).decode()
        assert rc == -1 and word in msg and "predict_thetas" in msg, (what, rc, msg)
        assert np.array_equal(dev.predict(Xq), good), what
    # lml, info and device_ms are optional
    assert dev._lib.gpry_predict_thetas(dev._h, vp(Tc), 3, vp(X), 2, vp(mean), None, None, None) == 0
    assert np.array_equal(mean, answer["mean"][:3, :2])
    assert np.array_equal(dev.predict(Xq), good) and same(dev.predict_thetas(T, Xq), answer)
    # the wrapper's shape checks
    with pytest.raises(ValueError):
        dev.predict_thetas(T[:, :-1], Xq)
    with pytest.raises(ValueError):
        dev.predict_thetas(T, Xq[:, :1])
    # no training set, and a training set without a kernel id
    fresh = _lib.Device(dev.device)
    try:
        rc = fresh._lib.gpry_predict_thetas(fresh._h, vp(Tc), 3, vp(X), 2, vp(mean), None, None, None)
        assert rc == -1 and "train" in fresh._lib.gpry_last_error(fresh._h).decode()
        fresh.set_train(X_, y_, a)
        rc = fresh._lib.gpry_predict_thetas(fresh._h, vp(Tc), 3, vp(X), 2, vp(mean), None, None, None)
        assert rc == -1 and "kernel id" in fresh._lib.gpry_last_error(fresh._h).decode()
    finally:
        fresh.close()
    # d > 32: such a model never reaches the call -- gpry_set_train refuses it, and the context keeps the model it had
    X33 = np.random.default_rng(0).uniform(0, 1, (40, 33))
    with pytest.raises(_lib.GpryHipError, match="32"):
        dev.set_train(X33, np.sin(X33.sum(1)), np.full(40, 1e-4))
    tm.load(dev, case)
    assert np.array_equal(dev.predict(Xq), good) and same(dev.predict_thetas(T, Xq), answer)


# ------------------------------------------------------------------------------------ the regressor
@pytest.mark.parametrize("N,d", [(130, 2), (333, 5)])
def test_hyper_spread_exact_end_to_end_on_a_fitted_regressor(N, d):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.mc import hyper_laplace, hyper_spread
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    b = np.array([[0.0, 1.0]] * d)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, d))
    # (less than one period across the box in every d: 333 points pin the length scales in five dimensions too -- with
    # sin(3 sum x) the fit at d = 5 ends on the lower bound of every length scale, where the mean is y_mean everywhere)
    y = np.sin(6.0 * X.mean(1)) + 0.1 * rng.standard_normal(N)
    kernel = Ck(1.0, [1e-3, 1e4]) * RBF([1.0] * d, [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=2, noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=7)
    gpr.append_to_data(X, y, fit_gpr=True)
    p = d + 2
    Xs = rng.uniform(0, 1, (256, d))
    ys = gpr.predict(Xs)
    theta0, lml0 = gpr.kernel_.theta.copy(), gpr.log_marginal_likelihood_value_
    lap = hyper_laplace(gpr)
    if not lap.negdef or not lap.free.all():
        lap = lap._replace(negdef=True, free=np.ones(p, dtype=bool), cov=0.01 * np.eye(p))
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    first = hyper_spread(gpr, Xs, ys, None, n_draws=16, seed=5, laplace=lap)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 256, l0)
    exact = hyper_spread(gpr, Xs, ys, None, n_draws=16, seed=5, laplace=lap, exact=True)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 2 * 256 + 17 * 256, l0 + 17)
    print(first, exact, f"first_order_miss {exact.first_order_miss:.3e}, theta_ess {exact.theta_ess:.2f}", sep="\n")
    assert first.exact is False and first.lml is None and exact.exact is True
    assert np.array_equal(first.dtheta, exact.dtheta) and np.array_equal(first.sigma_theta, exact.sigma_theta)
    assert not exact.failed.any() and exact.first_order_miss > 0 and exact.device_ms > 0
    # log r of the exact mode: differences of predict_thetas rows, bit for bit
    mean, lml, info = gpr.predict_thetas(Xs, np.vstack([lap.theta, lap.theta + exact.dtheta]), full=True)
    logr = mean[1:] - mean[0]
    assert exact.lml0 == lml[0] and np.array_equal(exact.lml, lml[1:]) and not info.any()
    assert exact.max_abs_logr == np.max(np.abs(logr))
    dlogZ = np.log(np.exp(logr).mean(axis=1))
    assert np.allclose(exact.dlogZ, dlogZ, rtol=0, atol=1e-12)
    assert np.array_equal(exact.sigma_theta_draws, mean[1:].std(axis=0))
    G = gpr.mean_theta_grad(Xs, full=True)[1]
    assert exact.first_order_miss == np.max(np.abs(logr - exact.dtheta.dot(G.T)))
    # the device's vector is the kernel's here ([log C, log l.., log w]): the mapped rows are the same call
    assert np.array_equal(gpr.kernel_.theta, lap.theta)
    # (... up to the rounding of exp and log on a theta's way through the kernel's clone)
    T3 = lap.theta + exact.dtheta[:3]
    rows = np.stack([np.asarray(gpr.kernel_.clone_with_theta(t).device_spec(d)[1], dtype=float) for t in T3])
    assert np.max(np.abs(rows - T3)) <= 8 * np.finfo(float).eps * np.max(np.abs(T3))
    assert np.array_equal(gpr.predict_thetas(Xs, T3)[0], gpr.predict_thetas(Xs, rows, full=True)[0])
    # a draw too small to move theta: log r = 0 and (256 equal weights sum to 1 exactly) dlogZ = 0, exactly
    tiny = hyper_spread(gpr, Xs, ys, None, n_draws=4, seed=5, laplace=lap._replace(cov=1e-60 * np.eye(p)), exact=True)
    assert np.array_equal(lap.theta + tiny.dtheta, np.tile(lap.theta, (4, 1))) and tiny.dtheta.any()
    assert tiny.max_abs_logr == 0.0 and np.all(tiny.dlogZ == 0.0) and np.all(tiny.lml == tiny.lml0)
    # nothing of the fitted model moved
    assert np.array_equal(gpr.predict(Xs), ys) and np.array_equal(gpr.kernel_.theta, theta0)
    assert gpr.log_marginal_likelihood_value_ == lml0
