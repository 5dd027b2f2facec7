"""Maximisation of the LogExp acquisition on the device (gpry_amd/csrc/maximize_acq.hip, gpry_amd/maximize.py:
maximize_acq, BatchOptimizer(acq_optimizer="device")): value and gradient against the one-point predict at every
(DP bucket, kernel id) instantiation and after a border update; every iteration of the walk table against the replay of
tests/tools/maximize_numpy.py; the invariants of the traces; first-order optimality checked from outside the kernel; a
start's result depends on its row alone; the optimiser value of BatchOptimizer; what the entry point refuses."""
import os
import sys
from copy import deepcopy

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed
from test_nested_gpu import _one_point, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import maximize_acq_numpy as man  # noqa: E402
import maximize_numpy as mn  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA_N = 0.1               # the noise level of the models below


def _check_value_and_gradient(gpr, X0, lo, hi, affine, ntrain, label):
    """max_iter = 0 on X0 (its last ``ntrain`` rows are training rows): the checks of the first two tests."""
    d = X0.shape[1]
    n = len(X0)
    zeta, baseline = float(d) ** -0.85, float(gpr.y_max)
    C, y_std = float(np.exp(gpr.kernel_.theta[0])), float(gpr._y_affine()[1])
    out = gpr.device.maximize_acq(lo, hi, X0, np.zeros(d, bool), np.eye(d), zeta, baseline, SIGMA_N, 0, 12, 1e-6, 0.0, -np.inf,
                                  hooks=True)
    np.testing.assert_array_equal(out["y"], _one_point(gpr, X0))
    np.testing.assert_array_equal(out["a"], gpr.device.debug_logexp(out["y"], out["sigma"], zeta, baseline, SIGMA_N))
    ref, sd = man.host_gradient(gpr, X0, lo, hi, zeta, SIGMA_N, 8.0 if affine else 1.0)
    err_var = np.max(np.abs(out["sigma"] ** 2 - sd ** 2))
    assert err_var <= 1e-9 * C * y_std ** 2, (label, err_var)
    q = sd ** 2 - SIGMA_N ** 2 >= 0.01 * C * y_std ** 2
    q[n - ntrain:] = False
    assert q.sum() >= n // 2, (label, q.sum())
    scale = np.max(np.abs(ref[q]))
    err = np.max(np.abs(out["G"][q] - ref[q]))
    print(f"{label}: {q.sum()} of {n} rows above the variance floor; max |G - ref| = {err:.3e} = {err / scale:.3e} max |ref|; "
          f"max |sigma^2 - std^2| = {err_var:.3e}")
    assert scale > 0 and err <= 1e-6 * scale, (label, err, scale)
    usable = np.isfinite(out["a"])
    assert usable[:n - ntrain].sum() >= n // 2
    np.testing.assert_array_equal(out["X"], X0)
    np.testing.assert_array_equal(out["iters"], 0)
    np.testing.assert_array_equal(out["ncalls"], 1)
    np.testing.assert_array_equal(out["ngrad"][usable], 1)
    assert set(out["status"][usable]) <= {mn.MAXITER, mn.CONVERGED_G}
    # the training rows: sigma^2 <= sigma_n^2 on them, no acquisition, no start
    assert np.all(np.isneginf(out["a"][n - ntrain:])) and np.all(out["status"][n - ntrain:] == mn.BAD_START)
    np.testing.assert_array_equal(out["status"][~usable], mn.BAD_START)
    np.testing.assert_array_equal(out["ngrad"][~usable], 0)
    assert np.all(np.isnan(out["G"][~usable]))
    np.testing.assert_array_equal(out["a_tr"][:, 0], out["a"])
    np.testing.assert_array_equal(out["G_tr"][:, 0], out["G"])
    assert out["U_tr"].shape == (n, 1, d) and out["nhalv_tr"].shape == (n, 0)
    return err / scale


# ---- 1. value and gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [100, 300, 1100])
@pytest.mark.parametrize("d", [2, 5, 9, 17])
@pytest.mark.parametrize("kid", [sw.RBF, sw.M12, sw.M32, sw.M52])
def test_value_and_gradient_are_the_one_point_predicts(kid, d, N):
    """max_iter = 0 on 22 uniform points of a box that is not the model's own and two training rows: y bit for bit the
    one-point predict, a bit for bit the sweep's LogExp of (y, sigma), sigma^2 within 1e-9 C y_std^2 of the one-point
    predict's, G within 1e-6 of the largest entry of the host gradient over the rows with sigma^2 - sigma_n^2 >= 0.01 C
    y_std^2.  Models with y_std = 1: see tests/tools/maximize_acq_numpy.py (value_model)."""
    affine = (kid + d + N // 1000) % 2 == 0
    gpr = _pushed(man.value_model(d, kid, N, affine).gpr())
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)
    rng = np.random.default_rng(kid + 10 * d)
    inside = np.flatnonzero(np.all((gpr.X_train >= lo) & (gpr.X_train <= hi), axis=1))
    X0 = np.ascontiguousarray(np.concatenate([rng.uniform(lo, hi, (22, d)), gpr.X_train[inside[:2]]]))
    _check_value_and_gradient(gpr, X0, lo, hi, affine, 2, f"kid={kid} d={d} N={N} affine={affine}")


# ---- 2. after a border update -----------------------------------------------------------------------------------------
def test_value_and_gradient_after_a_border_update_across_the_pad():
    """N = 126 + 4 rows by gpry_append_rows: N crosses the 128 pad, Np grows, and the checks of the first test hold
    against the one-point predict of the grown model."""
    d, affine = 3, True
    m = man.value_model(d, sw.M52, 130, affine, seed=7)
    X, y = m.X.copy(), m.y.copy()
    m.X, m.y = X[:126], y[:126]
    gpr = _pushed(m.gpr())
    assert gpr.device.N == 126
    before = getattr(gpr, "n_border_updates", 0)
    gpr.append_to_data(X[126:], y[126:], fit_gpr=False, fit_classifier=False)      # (as multi_add appends a lie)
    _pushed(gpr)
    assert gpr.device.N == 130 and getattr(gpr, "n_border_updates", 0) == before + 1
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)
    rng = np.random.default_rng(2)
    inside = np.flatnonzero(np.all((X >= lo) & (X <= hi), axis=1))
    X0 = np.ascontiguousarray(np.concatenate([rng.uniform(lo, hi, (22, d)), X[inside[-2:]]]))   # (the last rows: appended ones)
    _check_value_and_gradient(gpr, X0, lo, hi, affine, 2, "N=126+4")


# ---- 3. the walk ------------------------------------------------------------------------------------------------------
_WALKS = {}


def _walk(name):
    if name not in _WALKS:
        w = man.AcqWalk(name)
        gpr = _pushed(w.gpr)
        dev = gpr.device
        out = dev.maximize_acq(*w.args(), hooks=True)

        def value_of(X):
            # the kernel's own bits: a start depends on its row alone
            X = np.clip(np.ascontiguousarray(X), w.lo, w.hi)
            return dev.maximize_acq(w.lo, w.hi, X, w.fixed, w.H0, w.zeta, w.baseline, w.sigma_n, 0, 0, w.gtol, 0.0, -np.inf)["a"]

        rep = w.replay(out, value_of=value_of)
        _WALKS[name] = (w, gpr, out, rep)
    return _WALKS[name]


@pytest.mark.parametrize("name", man.ACQ_CASES)
def test_ascent_follows_the_replay_iteration_by_iteration(name):
    w, gpr, out, rep = _walk(name)
    keep = rep["ran"] & rep["keep"][:, :-1]
    step = keep & (out["nhalv_tr"] >= 0)
    du = float(np.max(np.abs(out["U_tr"][:, 1:] - rep["U_next"])[step], initial=0.0))
    left, ran = mn.left_out(rep)
    print(f"{name}: {left} of {ran} steps left out; max |dU| = {du:.3e} (tolerance {mn.REPLAY_TOL:.1e}); statuses "
          f"{np.bincount(out['status'], minlength=6)}; iterations {out['iters']}; halvings "
          f"{np.bincount(out['nhalv_tr'][out['nhalv_tr'] >= 0])}; resets {int(np.sum(out['reset_tr'] > 0))}")
    assert ran >= 2 * mn.N_STARTS and step.sum() > mn.N_STARTS
    assert du <= mn.REPLAY_TOL, (name, du)
    np.testing.assert_array_equal(out["nhalv_tr"][keep], rep["nhalv"][keep], err_msg=name)
    np.testing.assert_array_equal(out["reset_tr"][keep], rep["reset"][keep], err_msg=name)
    assert np.all(out["nhalv_tr"][~rep["ran"]] == -1) and np.all(out["reset_tr"][~rep["ran"]] == -1)
    whole = np.all(rep["keep"] | np.isnan(out["a_tr"]), axis=1)
    np.testing.assert_array_equal(out["iters"][whole], rep["end_iters"][whole], err_msg=name)
    np.testing.assert_array_equal(out["status"][whole], rep["end_status"][whole], err_msg=name)
    assert whole.sum() >= mn.N_STARTS // 2
    np.testing.assert_array_equal(out["ngrad"], out["iters"] + 1)
    np.testing.assert_array_equal(out["X"][:, w.fixed], w.X0[:, w.fixed])
    assert left <= mn.LEFT_OUT_CASE * ran, (name, left, ran)
    if w.target is not None:
        # the first full step of start 0 landed on the training row (a = -inf there) and was halved away
        assert out["nhalv_tr"][0, 0] >= 1


def test_left_out_share_of_the_walk_table():
    left = ran = 0
    for name in man.ACQ_CASES:
        a, b = mn.left_out(_walk(name)[3])
        left, ran = left + a, ran + b
    print(f"{left} of {ran} steps left out")
    assert left <= mn.LEFT_OUT_TABLE * ran, (left, ran)


# ---- 4. invariants on the traces --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", man.ACQ_CASES)
def test_invariants_of_the_traces(name):
    w, gpr, out, _ = _walk(name)
    ev = ~np.isnan(out["a_tr"])
    np.testing.assert_array_equal(np.sum(ev, axis=1), out["iters"] + 1)
    started = out["status"] != mn.BAD_START
    assert started.sum() >= mn.N_STARTS // 2
    for c in np.flatnonzero(started):
        assert np.all(np.diff(out["a_tr"][c, :out["iters"][c] + 1]) >= 0), (name, c)
    assert np.all(np.isfinite(out["a_tr"][started][ev[started]])) and np.all(np.isfinite(out["a"][started]))
    U = out["U_tr"][ev]
    assert np.all((U >= 0) & (U <= 1)) and np.all((out["X"] >= w.lo) & (out["X"] <= w.hi))
    X = mn.trace_points(man.as_mean_trace(out), w.lo, w.hi, w.X0)
    np.testing.assert_array_equal(X[ev][:, w.fixed], np.repeat(w.X0[:, None], X.shape[1], axis=1)[ev][:, w.fixed])
    np.testing.assert_array_equal(out["X"], X[np.arange(len(w.X0)), out["iters"]])
    np.testing.assert_array_equal(out["ngrad"][started], out["iters"][started] + 1)
    np.testing.assert_array_equal(out["a"], out["a_tr"][np.arange(len(w.X0)), out["iters"]])
    np.testing.assert_array_equal(out["y"], _one_point(gpr, out["X"]))
    assert np.all(out["ncalls"] >= 1 + out["iters"])


# ---- 5. first-order check from outside the kernel ---------------------------------------------------------------------
def test_a_start_that_ends_on_the_gradient_test_is_stationary_for_the_host_gradient():
    d, affine, gtol = 3, True, 1e-5
    gpr = _pushed(man.value_model(d, sw.M52, 300, affine).gpr())
    bounds = gpr.bounds
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    zeta, baseline = float(d) ** -0.85, float(gpr.y_max)
    X0 = np.ascontiguousarray(np.random.default_rng(5).uniform(lo, hi, (32, d)))
    from gpry_amd.maximize import acq_h0
    args = (lo, hi, X0, np.zeros(d, bool), acq_h0(gpr, None, lo, hi), zeta, baseline, SIGMA_N)
    a0 = gpr.device.maximize_acq(*args, 0, 12, gtol, 0.0, -np.inf)["a"]
    out = gpr.device.maximize_acq(*args, 200, 12, gtol, 0.0, -np.inf)
    conv = out["status"] == mn.CONVERGED_G
    print(f"statuses {np.bincount(out['status'], minlength=6)}, iterations {out['iters']}, evaluations {out['ncalls']}")
    assert conv.sum() >= 8
    ref, _ = man.host_gradient(gpr, out["X"][conv], lo, hi, zeta, SIGMA_N, 8.0)
    U = (out["X"][conv] - lo) / (hi - lo)
    free = ~((U == 0) & (ref <= 0)) & ~((U == 1) & (ref >= 0))
    worst = np.max(np.where(free, np.abs(ref), 0.0), axis=1)
    print(f"largest free component of the host gradient at the CONVERGED_G end points: {worst.max():.3e}")
    assert np.all(worst <= gtol + 1e-6 * np.max(np.abs(ref), axis=1))
    assert np.all(out["a"][conv] >= a0[conv])


# ---- 6. row independence ----------------------------------------------------------------------------------------------
def test_rows_of_a_call_do_not_depend_on_the_other_rows():
    w, gpr, _, _ = _walk("d=3 M52 N=300 one fixed")
    full = gpr.device.maximize_acq(*w.args(), hooks=True)
    a = list(w.args())
    a[2] = np.ascontiguousarray(w.X0[[3, 7]])
    two = gpr.device.maximize_acq(*a, hooks=True)
    assert np.sum(full["iters"][[3, 7]]) > 0
    for key in ("X", "a", "y", "sigma", "G", "iters", "ncalls", "ngrad", "status", "U_tr", "a_tr", "G_tr", "nhalv_tr", "reset_tr"):
        np.testing.assert_array_equal(full[key][[3, 7]], two[key], err_msg=key)


# ---- 7. BatchOptimizer ------------------------------------------------------------------------------------------------
def test_batch_optimizer_with_the_device_optimiser():
    from gpry_amd.gp_acquisition import BatchOptimizer
    from gpry_amd.preprocessing import Normalize_bounds
    from gpry_amd.proposal import UniformProposer
    m = sw.Model(2, sw.M52, 60, seed=4)
    m.theta = np.log([4.0, 0.15, 0.15])
    bounds = m.bounds
    kw = dict(n_restarts_optimizer=10, n_repeats_propose=2, verbose=0)
    res = {}
    for opt in ("device", "fmin_l_bfgs_b"):
        gpr = m.gpr()
        acq = BatchOptimizer(bounds, preprocessing_X=Normalize_bounds(bounds), acq_optimizer=opt,
                             proposer=UniformProposer(bounds), **kw)
        starts, orig = [], acq._starting_point

        def spy(g, i, b, rng, orig=orig, acq=acq, starts=starts):
            x0, settled = orig(g, i, b, rng)
            starts.append(float(np.ravel(acq.acq_func(np.atleast_2d(acq.preprocessing_X.inverse_transform(x0)), g))[0]))
            return x0, settled

        acq._starting_point = spy
        rng = np.random.default_rng(5)
        Xo, yl, av = acq.multi_add(gpr, n_points=3, rng=rng)
        res[opt] = dict(gpr=gpr, acq=acq, X=Xo, y=yl, a=av, after=rng.random(), starts=np.array(starts).reshape(3, -1))
    r = res["device"]
    acq, gpr = r["acq"], r["gpr"]
    assert acq.stats["device_optimizer"] is True and acq.stats["border_updates"] == 2 and gpr.n == 60
    assert acq.stats["device_ms"] > 0 and sum(acq.stats["device_status"].values()) == 30
    assert "device_optimizer" not in res["fmin_l_bfgs_b"]["acq"].stats
    assert np.all((r["X"] >= bounds[:, 0]) & (r["X"] <= bounds[:, 1])) and np.all(np.isfinite(r["a"]))
    g2 = deepcopy(gpr)
    for p in range(3):
        a = float(np.ravel(acq.acq_func(r["X"][p][None, :], g2))[0])
        assert abs(a - r["a"][p]) <= 1e-6, (p, a, r["a"][p])
        assert r["a"][p] >= np.max(r["starts"][p][np.isfinite(r["starts"][p])]) - 1e-6
        g2.append_to_data(r["X"][p][None, :], r["y"][p:p + 1], fit_gpr=False, fit_classifier=False)
    # both optimisers consume the generator in _starting_point only
    assert r["after"] == res["fmin_l_bfgs_b"]["after"]
    print(f"best acquisition per proposal: device {r['a']}, fmin_l_bfgs_b {res['fmin_l_bfgs_b']['a']}; device status "
          f"{acq.stats['device_status']}, {acq.stats['device_ms']:.2f} ms on the device")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_with_a_message_and_runs_nothing():
    from gpry_amd._lib import GpryHipError
    w, gpr, _, _ = _walk("d=3 M52 N=300 one fixed")
    ok = list(w.args())
    gpr.device.maximize_acq(*ok)
    for pos, bad, word in ((7, -0.1, "sigma_n"), (7, np.nan, "sigma_n"), (5, np.inf, "zeta"), (6, np.nan, "baseline"),
                           (8, -1, "max_iter"), (8, 100001, "max_iter"), (9, -1, "max_halvings"), (10, -1.0, "gtol"),
                           (11, np.inf, "ftol"), (0, w.hi, "bounds"), (4, np.full((3, 3), np.nan), "H0")):
        a = list(ok)
        a[pos] = bad
        with pytest.raises(GpryHipError, match=word):
            gpr.device.maximize_acq(*a)
    # hooks half given: through the C interface itself
    import ctypes as C
    dev = gpr.device
    n, d = w.X0.shape
    buf = lambda *s, t=np.float64: np.zeros(s, t)      # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731
    X, a_, y_, s_, G = buf(n, d), buf(n), buf(n), buf(n), buf(n, d)
    it, nc, ng, st = buf(n, t=np.int32), buf(n, t=np.int64), buf(n, t=np.int64), buf(n, t=np.int32)
    U = buf(n, 4, d)
    st[:] = -7
    fx = w.fixed.astype(np.uint8)
    rc = dev._lib.gpry_maximize_acq(dev._h, p(w.lo), p(w.hi), p(w.X0), n, p(fx), p(w.H0), w.zeta, w.baseline,
                                    w.sigma_n, 3, 12, 1e-6, 0.0, -np.inf, p(X), p(a_), p(y_), p(s_), p(G), p(it), p(nc), p(ng),
                                    p(st), p(U), None, None, None, None, None)
    assert rc == -1 and np.all(st == -7)
    with pytest.raises(GpryHipError, match="hooks"):
        dev._check(rc, "gpry_maximize_acq")


def test_a_model_above_4096_padded_rows_is_refused():
    from gpry_amd._lib import GpryHipError
    m = sw.Model(2, sw.M52, 4100, normalize_y=False, noise_level=0.1)
    gpr = _pushed(m.gpr())
    lo, hi = m.bounds[:, 0].copy(), m.bounds[:, 1].copy()
    with pytest.raises(GpryHipError, match="4096"):
        gpr.device.maximize_acq(lo, hi, np.zeros((2, 2)), np.zeros(2, bool), np.eye(2), 0.5, 0.0, 0.1, 3, 12, 1e-6, 0.0, -np.inf)


# ---- the public interface ---------------------------------------------------------------------------------------------
def test_maximize_acq_of_the_mc_namespace_and_the_y_std_of_the_gradient():
    """maximize_acq on a model with normalised y (y_std != 1): the result is self-consistent, n_eval grows by ncalls, and
    the kernel's gradient is the central difference of the kernel's own value (h = 1e-4 of the box: the truncation error
    h^2 a''' / 6 and the rounding 1e-15 |a| / h are both far below 1e-5 of the gradient for these smooth models)."""
    from gpry_amd.mc import maximize_acq
    m = sw.Model(3, sw.M52, 300, seed=3)
    m.theta = np.log([4.0, 0.1, 0.1, 0.1])
    gpr = m.gpr()
    before = gpr.n_eval
    r = maximize_acq(gpr, nstarts=16, rng=7, max_iter=50)
    assert gpr.n_eval - before == r.ncalls.sum()
    assert r.X_all.shape == (16, 3) and np.isfinite(r.acq) and r.acq == np.max(r.acq_all[np.isfinite(r.acq_all)])
    assert float(gpr._y_affine()[1]) != 1.0
    from gpry_amd.acquisition_functions import LogExp
    host = LogExp(dimension=3)(r.X_all, gpr)
    fin = np.isfinite(r.acq_all)
    assert np.max(np.abs(host[fin] - r.acq_all[fin])) <= 1e-6
    lo, hi = gpr.bounds[:, 0].copy(), gpr.bounds[:, 1].copy()
    zeta, sn = float(LogExp(dimension=3).zeta), float(gpr.noise_level)
    X = np.ascontiguousarray(np.random.default_rng(1).uniform(lo, hi, (8, 3)))
    call = lambda Z: gpr.device.maximize_acq(lo, hi, np.ascontiguousarray(Z), np.zeros(3, bool), np.eye(3), zeta,  # noqa: E731
                                             float(gpr.y_max), sn, 0, 0, 1e-6, 0.0, -np.inf)
    G = call(X)["G"]
    h = 1e-4
    for k in range(3):
        e = np.zeros(3)
        e[k] = h * (hi[k] - lo[k])
        fd = (call(X + e)["a"] - call(X - e)["a"]) / (2 * h)
        ok = np.isfinite(fd) & np.isfinite(G[:, k])
        assert ok.sum() >= 4
        assert np.max(np.abs(fd - G[:, k])[ok]) <= 1e-5 * np.max(np.abs(G[ok])), (k, fd, G[:, k])
