"""Maximisation of the surrogate's mean on the device (gpry_amd/csrc/maximize.hip + gpry_amd/maximize.py): the gradient
and the value the kernel works with are the one-point predict's at every (DP bucket, kernel id) instantiation; every
traced y equals gpr.predict of its row bit for bit and never decreases; every iteration follows the replay of
tests/tools/maximize_numpy.py; no iterate leaves the box or lies on gated ground and fixed coordinates keep their bits;
a start that ends on the gradient test satisfies it; a start's result depends on its row alone; maximize_gp and
profile_gp agree with the same host code on the oracle; both are in gpry_amd.mc's namespace."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed, _starts
from test_nested_gpu import _one_point, _parity_cases, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import maximize_numpy as mn  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu


def _h0(gpr, bounds):
    """maximize_gp's H0: the training set's weighted covariance in the unit cube, ridged."""
    from gpry_amd.maximize import _h0, _usable
    lo, hi = bounds[:, 0], bounds[:, 1]
    Xt, yt = _usable(gpr.X_train, gpr.y_train, lo, hi, gpr.minus_inf_value)
    return _h0(None, Xt, yt, hi - lo)


# ---- gradient and value -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [100, 1100, 2500])
@pytest.mark.parametrize("d", [2, 5, 9, 17])
@pytest.mark.parametrize("kid", [sw.RBF, sw.M12, sw.M32, sw.M52])
def test_gradient_and_value_are_the_one_point_predicts(kid, d, N):
    """max_iter = 0: G against span x gpr.predict(x[None], return_mean_grad=True), within 1e-7 of its largest entry
    (predict's gradient is taken in the model's transformed coordinates: with the x-affine map, every other case, the
    raw-coordinate gradient is that over the map's span, here 8), and y bit for bit."""
    affine = (kid + d + N // 1000) % 2 == 0
    model = sw.Model(d, kid, N, affine=affine, seed=N + d)
    gpr = _pushed(model.gpr())
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)              # (not the model's own box)
    rng = np.random.default_rng(kid + 10 * d)
    X0 = np.ascontiguousarray(np.concatenate([gpr.X_train[rng.choice(N, 8)], rng.uniform(lo, hi, (16, d))]))
    X0 = np.clip(X0, lo, hi)
    n = len(X0)
    out = gpr.device.maximize_mean(lo, hi, X0, np.full(n, np.nan), np.zeros(d, bool), np.eye(d), 0, 12, 1e-6, 0.0, -np.inf,
                                   hooks=True)
    ref = np.array([np.ravel(gpr.predict(x[None, :], return_mean_grad=True)[1]) for x in X0])
    ref = ref * (hi - lo) / (8.0 if affine else 1.0)
    err = np.max(np.abs(out["G"] - ref))
    print(f"kid={kid} d={d} N={N} affine={affine}: max |G - ref| = {err:.3e}, max |ref| = {np.max(np.abs(ref)):.3e}")
    assert np.max(np.abs(ref)) > 0
    assert err <= 1e-7 * np.max(np.abs(ref))
    np.testing.assert_array_equal(out["y"], _one_point(gpr, X0))
    np.testing.assert_array_equal(out["X"], X0)
    np.testing.assert_array_equal(out["iters"], 0)
    np.testing.assert_array_equal(out["ngrad"], 1)
    np.testing.assert_array_equal(out["ncalls"], 1)
    assert set(out["status"]) <= {mn.MAXITER, mn.CONVERGED_G}
    assert out["U_tr"].shape == (n, 1, d) and out["nhalv_tr"].shape == (n, 0)
    np.testing.assert_array_equal(out["G_tr"][:, 0], out["G"])
    np.testing.assert_array_equal(out["y_tr"][:, 0], out["y"])
    np.testing.assert_array_equal(out["U_tr"][:, 0], (X0 - lo) / (hi - lo))


# ---- every traced y ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_traced_y_equals_one_point_predict_and_never_decreases(case):
    gpr, bounds = dict(_parity_cases())[case]()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n, d = 12, len(bounds)
    X0 = _starts(gpr, n, 3)
    out = gpr.device.maximize_mean(lo, hi, X0, np.full(n, np.nan), np.zeros(d, bool), _h0(gpr, bounds), 10, 12, 1e-6, 0.0,
                                   gpr.minus_inf_value, hooks=True)
    X = mn.trace_points(out, lo, hi, X0)
    ev = ~np.isnan(out["y_tr"])
    np.testing.assert_array_equal(np.sum(ev, axis=1), out["iters"] + 1)
    np.testing.assert_array_equal(out["y_tr"][ev], _one_point(gpr, X[ev]))
    np.testing.assert_array_equal(out["y"], _one_point(gpr, out["X"]))
    np.testing.assert_array_equal(out["X"], X[np.arange(n), out["iters"]])
    y0 = _one_point(gpr, X0)
    ok = out["status"] != mn.BAD_START
    assert ok.sum() >= n // 2
    for c in np.flatnonzero(ok):
        assert np.all(np.diff(out["y_tr"][c, :out["iters"][c] + 1]) >= 0), (case, c)
    assert np.all(out["y"][ok] >= y0[ok])
    print(f"{case}: statuses {np.bincount(out['status'], minlength=6)}, iterations {out['iters']}")
    assert np.sum(out["iters"]) > 0


# ---- the walk ---------------------------------------------------------------------------------------------------------
_WALKS = {}


def _walk(name):
    if name not in _WALKS:
        w = mn.Walk(name)
        gpr = _pushed(w.gpr)
        out = gpr.device.maximize_mean(*w.args(), hooks=True)
        rep = w.replay(out, value_of=lambda X: _one_point(gpr, X))
        _WALKS[name] = (w, gpr, out, rep)
    return _WALKS[name]


@pytest.mark.parametrize("name", mn.MAX_CASES)
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
    # an iteration whose search never ran has no trace
    assert np.all(out["nhalv_tr"][~rep["ran"]] == -1) and np.all(out["reset_tr"][~rep["ran"]] == -1)
    # where every decision of a start is kept, the replay sees it end where it ended
    whole = np.all(rep["keep"] | np.isnan(out["y_tr"]), axis=1)
    np.testing.assert_array_equal(out["iters"][whole], rep["end_iters"][whole], err_msg=name)
    np.testing.assert_array_equal(out["status"][whole], rep["end_status"][whole], err_msg=name)
    assert whole.sum() >= mn.N_STARTS // 2
    np.testing.assert_array_equal(out["ngrad"], out["iters"] + 1)
    np.testing.assert_array_equal(out["X"][:, w.fixed], w.X0[:, w.fixed])
    assert left <= mn.LEFT_OUT_CASE * ran, (name, left, ran)


def test_left_out_share_of_the_walk_table():
    left = ran = 0
    for name in mn.MAX_CASES:
        a, b = mn.left_out(_walk(name)[3])
        left, ran = left + a, ran + b
    print(f"{left} of {ran} steps left out")
    assert left <= mn.LEFT_OUT_TABLE * ran, (left, ran)


# ---- box and gates ----------------------------------------------------------------------------------------------------
def test_no_iterate_outside_the_box_or_on_gated_ground_and_fixed_coordinates_keep_their_bits():
    gpr, bounds = _svm_model()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n = 32
    X0 = _starts(gpr, n, 5)
    fixed = np.array([False, True, False])
    out = gpr.device.maximize_mean(lo, hi, X0, np.full(n, np.nan), fixed, 8.0 * _h0(gpr, bounds), 20, 12, 1e-6, 0.0,
                                   gpr.minus_inf_value, hooks=True)
    X = mn.trace_points(out, lo, hi, X0)
    ev = ~np.isnan(out["y_tr"])
    Xe = X[ev]
    assert np.all((Xe >= lo) & (Xe <= hi)) and np.all((out["X"] >= lo) & (out["X"] <= hi))
    ok = out["status"] != mn.BAD_START
    assert ok.sum() > n // 2 and np.sum(out["iters"]) > n
    ye = gpr.predict(X[ok][ev[ok]])
    assert np.all(np.isfinite(ye)) and np.all(np.isfinite(out["y"][ok]))
    np.testing.assert_array_equal(out["y_tr"][ev], _one_point(gpr, Xe))
    np.testing.assert_array_equal(out["X"][:, fixed], X0[:, fixed])
    np.testing.assert_array_equal(X[ev][:, fixed], np.repeat(X0[:, None], X.shape[1], axis=1)[ev][:, fixed])
    # the long first steps met the gates or the walls: some searches backed off
    assert np.sum(out["nhalv_tr"] > 0) > 0
    assert np.all(out["ncalls"] >= 1 + out["iters"])


# ---- KKT at the end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [False, True])
def test_a_start_that_ends_on_the_gradient_test_satisfies_it(cut):
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    bounds = bounds.copy()
    if cut:
        bounds[0, 1] = 0.0                       # the wall x_0 = 0 cuts the peak (0.3) off
    lo, hi = bounds[:, 0], bounds[:, 1]
    gtol = 1e-5
    from gpry_amd.maximize import _usable
    X0 = np.ascontiguousarray(_usable(gpr.X_train, gpr.y_train, lo, hi, -np.inf)[0][:24])
    fixed = np.array([False, False, True])
    out = gpr.device.maximize_mean(lo, hi, X0, np.full(24, np.nan), fixed, _h0(gpr, bounds), 100, 12, gtol, 0.0, -np.inf)
    conv = out["status"] == mn.CONVERGED_G
    print(f"cut={cut}: statuses {np.bincount(out['status'], minlength=6)}, iterations {out['iters']}")
    assert conv.sum() >= 6
    U = (out["X"] - lo) / (hi - lo)
    G = out["G"]
    free = ~fixed & ~((U == 0) & (G <= 0)) & ~((U == 1) & (G >= 0))
    assert np.all(np.max(np.where(free, np.abs(G), 0.0), axis=1)[conv] <= gtol)
    if cut:
        assert np.all(out["X"][conv][:, 0] == 0.0) and np.all(G[conv][:, 0] > gtol)


# ---- independence -----------------------------------------------------------------------------------------------------
def test_same_bits_on_two_contexts_in_split_calls_and_at_any_position():
    from test_nested_gpu import _fixed, _gauss_ll
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, theta)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    assert gpr2.device is not gpr.device
    H0 = _h0(_pushed(gpr), bounds)
    _pushed(gpr2)
    k = 16
    X0 = _starts(gpr, 2 * k, 8)
    fixed = np.array([False, False, True, False])
    call = lambda dev, X: dev.maximize_mean(bounds[:, 0], bounds[:, 1], X, np.full(len(X), np.nan), fixed, H0, 8, 12,  # noqa: E731
                                            1e-6, 0.0, -np.inf, hooks=True)
    keys = ("X", "y", "G", "iters", "ncalls", "ngrad", "status", "U_tr", "y_tr", "G_tr", "nhalv_tr", "reset_tr")
    a, b = call(gpr.device, X0), call(gpr2.device, X0)
    h1, h2 = call(gpr.device, X0[:k]), call(gpr.device, X0[k:])
    perm = np.random.default_rng(0).permutation(2 * k)
    p = call(gpr.device, np.ascontiguousarray(X0[perm]))
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a[key], np.concatenate([h1[key], h2[key]]), err_msg=key)
        np.testing.assert_array_equal(a[key][perm], p[key], err_msg=key)
    assert np.sum(a["iters"]) > 2 * k
    # the traces are a hook: the results without them are the same bits, and a given y0 is not evaluated again
    c = gpr.device.maximize_mean(bounds[:, 0], bounds[:, 1], X0, a["y_tr"][:, 0], fixed, H0, 8, 12, 1e-6, 0.0, -np.inf)
    for key in keys[:7]:
        if key != "ncalls":
            np.testing.assert_array_equal(a[key], c[key], err_msg=key)
    np.testing.assert_array_equal(a["ncalls"], c["ncalls"] + 1)
    assert "U_tr" not in c


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mn.E2E_MODELS))
def test_maximize_gp_and_profile_gp_agree_with_the_host_code_on_the_oracle(name):
    m, ogpr = mn.e2e_oracle(name)
    ref = mn.e2e_results(ogpr, m.d)
    gpr = m.gpr()
    before = gpr.n_eval
    got = mn.e2e_results(gpr, m.d)
    tol = 2 * m.tol()
    print(f"{name}: best y {got[0].y:.9g} (oracle {ref[0].y:.9g}); max profile difference "
          f"{np.max(np.abs(got[1].y - ref[1].y)):.3e} (1-D), {np.max(np.abs(got[2].y - ref[2].y)):.3e} (2-D); tolerance "
          f"{tol:.3e}; device {1e3 * (got[0].device_s + got[1].device_s + got[2].device_s):.1f} ms")
    assert abs(got[0].y - ref[0].y) <= tol
    assert got[1].y.shape == (9,) and got[2].y.shape == (9,)
    assert np.max(np.abs(got[1].y - ref[1].y)) <= tol
    assert np.max(np.abs(got[2].y - ref[2].y)) <= tol
    assert gpr.n_eval - before == got[0].ncalls.sum() + got[1].ncalls + got[2].ncalls
    np.testing.assert_array_equal(got[1].X[:, 0], mn.E2E_GRID_1D)
    np.testing.assert_array_equal(got[2].X[:, [0, m.d - 1]], mn.E2E_GRID_2D)
    np.testing.assert_array_equal(got[0].y_all, _one_point(gpr, got[0].X_all))
    np.testing.assert_array_equal(got[1].y, _one_point(gpr, got[1].X))


# ---- the public interface ---------------------------------------------------------------------------------------------
def test_mc_namespace_has_both_and_bad_arguments_are_refused_with_a_message():
    from gpry_amd._lib import GpryHipError
    from gpry_amd.mc import maximize_gp, profile_gp
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    r = maximize_gp(gpr, bounds=bounds, nstarts=8)
    assert r.X_all.shape == (8, 3) and np.isfinite(r.y) and r.y >= np.max(gpr.y_train[np.isfinite(gpr.y_train)]) - 1e-3
    p = profile_gp(gpr, 1, [0.0, 0.3], bounds=bounds, nstarts=4)
    assert p.y.shape == (2,) and np.all(np.isfinite(p.y)) and np.all(p.y <= r.y + 1e-9)
    X0 = _starts(gpr, 4, 1)

    def call(lo=bounds[:, 0], H0=np.eye(3), max_iter=3, max_halvings=12, gtol=1e-6, ftol=0.0):
        return gpr.device.maximize_mean(lo, bounds[:, 1], X0, np.full(4, np.nan), np.zeros(3, bool), H0, max_iter, max_halvings,
                                        gtol, ftol, -np.inf)

    call()
    for kw, word in ((dict(max_iter=-1), "max_iter"), (dict(max_halvings=-1), "max_halvings"), (dict(gtol=-1.0), "gtol"),
                     (dict(gtol=np.nan), "gtol"), (dict(ftol=np.inf), "ftol"), (dict(lo=bounds[:, 1]), "bounds"),
                     (dict(H0=np.full((3, 3), np.nan)), "H0")):
        with pytest.raises(GpryHipError, match=word):
            call(**kw)
    with pytest.raises(ValueError):
        gpr.device.maximize_mean(bounds[:, 0], bounds[:, 1], X0, np.full(4, np.nan), np.zeros(2, bool), np.eye(3), 3, 12, 1e-6,
                                 0.0, -np.inf)
