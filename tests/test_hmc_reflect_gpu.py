"""Reflection at the box walls in the device's HMC (gpry_hmc_chains_reflect, hmc_chain_kernel<DP, KID, true> in
gpry_amd/csrc/hmc.hip; gpry_amd/hmc.py, gpry_amd/mc.py): with reflect = 0 the new entry is gpry_hmc_chains bit for bit, and so
is reflect = 1 in a box no chain touches; every trajectory follows the host reference of
tests/tools/hmc_reflect_numpy.py on the oracle, reflections counted; every recorded y is gpr.predict of its row bit for bit,
no state leaves the box or lies on gated ground, and nothing but the cap cuts a trajectory short; the same seed gives the
same bits on two contexts, for any number of chains and when a call goes on from another; run_hmc(reflect=True) and run_mcmc
agree on a surrogate that fills its box; mc_sample_from_gp runs it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_hmc_gpu import _chain_means, _factor
from test_mcmc_gpu import _pushed, _starts
from test_nested_gpu import _one_point, _parity_cases, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hmc_reflect_numpy as hr  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

K, S = hr.N_CHAINS, hr.N_TRAJ
KEYS = ("X", "y", "X_last", "y_last", "naccept", "ncalls", "ngrad", "X_prop", "y_prop", "dH_prop", "G0")


def _entry(dev, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, reflect, max_reflect):
    """gpry_hmc_chains_reflect itself, hooks on, whatever ``reflect`` (``hmc_chains`` takes the old entry without it)."""
    from gpry_amd._lib import _f64, _ptr
    d = dev.d
    lo, hi, X0 = _f64(lo, (d,)), _f64(hi, (d,)), _f64(X0)
    n = len(X0)
    y0, Lp = _f64(y0, (n,)), _f64(Lp, (d, d))
    nrec = nsteps // thin
    out = dict(X=np.empty((n, nrec, d)), y=np.empty((n, nrec)), X_last=np.empty((n, d)), y_last=np.empty(n),
               naccept=np.zeros(n, np.int64), ncalls=np.zeros(n, np.int64), ngrad=np.zeros(n, np.int64),
               X_prop=np.empty((n, nsteps, d)), y_prop=np.empty((n, nsteps)), dH_prop=np.empty((n, nsteps)),
               G0=np.empty((n, d)), nreflect=np.full(n, -1, np.int64))
    ms = C.c_double(0.0)
    dev._check(dev._lib.gpry_hmc_chains_reflect(
        dev._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), n, _ptr(Lp), float(eps), int(nleap), float(T), float(minus_inf_value),
        int(seed), int(batch), nsteps, thin, _ptr(out["X"]), _ptr(out["y"]), _ptr(out["X_last"]), _ptr(out["y_last"]),
        _ptr(out["naccept"]), _ptr(out["ncalls"]), _ptr(out["ngrad"]), _ptr(out["X_prop"]), _ptr(out["y_prop"]),
        _ptr(out["dH_prop"]), _ptr(out["G0"]), int(reflect), int(max_reflect), _ptr(out["nreflect"]), C.byref(ms)),
        "gpry_hmc_chains_reflect")
    return out


# ---- reflect off, and on where it does nothing ------------------------------------------------------------------------
# one model per DP bucket: (d, kernel id, N)
_BUCKETS = [(3, sw.M52, 600), (8, sw.M12, 1100), (16, sw.RBF, 300), (32, sw.M32, 300)]


@pytest.mark.parametrize("d,kid,N", _BUCKETS)
def test_the_new_entry_with_reflect_off_is_the_old_entry_bit_for_bit(d, kid, N):
    model = sw.Model(d, kid, N, seed=N + d)
    gpr = _pushed(model.gpr())
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)              # (not the model's own box: trajectories leave it)
    n, steps = 12, 10
    X0 = np.clip(_starts(gpr, n, 3), lo + 1e-3, hi - 1e-3)
    args = (lo, hi, X0, np.full(n, np.nan), 2.0 * _factor(gpr, model.bounds), 0.4, 4, 1.0, gpr.minus_inf_value, 77, 1,
            steps, 1)
    old = gpr.device.hmc_chains(*args, hooks=True)
    new = _entry(gpr.device, *args, 0, 0)                   # (max_reflect is not read)
    assert "nreflect" not in old
    for k in KEYS:
        np.testing.assert_array_equal(old[k], new[k], err_msg=k)
    np.testing.assert_array_equal(new["nreflect"], 0)
    assert old["naccept"].sum() > 0
    # reflect on, in a box no chain touches: the same bits, and no reflection
    wide = (np.full(d, -60.0), np.full(d, 60.0)) + args[2:4] + (args[4] / 15.0,) + args[5:]
    a = gpr.device.hmc_chains(*wide, hooks=True)
    b = gpr.device.hmc_chains(*wide, hooks=True, reflect=True)
    assert not np.isnan(a["y_prop"]).any() and a["naccept"].sum() > 0
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(b["nreflect"], 0)


# ---- the walk ---------------------------------------------------------------------------------------------------------
_WALKS = {}


def _walk(name):
    if name not in _WALKS:
        w = hr.Walk(name)
        _WALKS[name] = (w, w.trace())
    return _WALKS[name]


@pytest.mark.parametrize("name", hr.REFLECT_CASES)
def test_reflecting_chain_follows_the_reference_trajectory_by_trajectory(name):
    w, tr = _walk(name)
    gpr = _pushed(w.gpr)
    out = gpr.device.hmc_chains(*w.args(), 1, hooks=True, reflect=True, max_reflect=w.max_reflect)
    span = w.hi - w.lo
    np.testing.assert_array_equal(out["y"].ravel(), _one_point(gpr, out["X"].reshape(-1, w.model.d)))
    g0 = w.grad_x(w.X0) * span
    assert np.max(np.abs(out["G0"] - g0)) <= 1e-7 * np.max(np.abs(g0))
    assert np.all((out["X_prop"] >= w.lo) & (out["X_prop"] <= w.hi))
    X_prev = w.X0
    worst = 0.0
    for s in range(S):
        keep = tr.keep(s)
        where = f"{name}, trajectory {s}: {int(np.sum(~keep))} of {K} chains left out"
        U = (out["X_prop"][:, s] - w.lo) / span
        du = np.max(np.abs(U[keep] - tr.U[s][keep]), initial=0.0)
        worst = max(worst, du)
        print(f"{where}; max |du| = {du:.3e}")
        assert du <= hr.POS_TOL, (where, du)
        np.testing.assert_array_equal(np.isnan(out["y_prop"][:, s])[keep], np.isnan(tr.y[s])[keep], err_msg=where)
        moved = np.any(out["X"][:, s] != X_prev, axis=1)
        np.testing.assert_array_equal(moved[keep], tr.accepted[s][keep], err_msg=where)
        ev = keep & ~np.isnan(tr.y[s]) & np.isfinite(tr.y[s])
        assert np.max(np.abs(out["y_prop"][:, s][ev] - tr.y[s][ev]), initial=0.0) <= w.model.tol(), where
        assert np.max(np.abs(out["dH_prop"][:, s][ev] - tr.dH[s][ev]), initial=0.0) <= 2 * w.model.tol() / w.T + 1e-9, where
        X_prev = out["X"][:, s]
    keep = tr.keep(S - 1)
    np.testing.assert_array_equal(out["ncalls"][keep], tr.ncalls[S - 1][keep])
    np.testing.assert_array_equal(out["ngrad"][keep], tr.ngrad[S - 1][keep])
    np.testing.assert_array_equal(out["naccept"][keep], tr.accepted.sum(axis=0)[keep])
    np.testing.assert_array_equal(out["nreflect"][keep], tr.nreflect[S - 1][keep])
    left = int(np.sum(~keep))
    print(f"{name}: compared {K - left} of {K} chains over {S} trajectories; max |du| = {worst:.3e} "
          f"(tolerance {hr.POS_TOL:.1e}); {int(tr.accepted.sum())} accepted, {int(out['nreflect'].sum())} reflections "
          f"(reference: {int(tr.nreflect[S - 1].sum())})")
    assert left <= hr.LEFT_OUT_CASE * K, (name, left)
    assert out["nreflect"][keep].sum() > 0


def test_left_out_share_of_the_reflecting_walk_table():
    left = sum(int(np.sum(~_walk(name)[1].keep(S - 1))) for name in hr.REFLECT_CASES)
    assert left <= hr.LEFT_OUT_TABLE * K * len(hr.REFLECT_CASES), left


# ---- recorded y, box and gates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_recorded_y_of_a_reflecting_chain_equals_one_point_predict(case):
    gpr, bounds = dict(_parity_cases())[case]()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n, steps, d = 12, 20, len(bounds)
    X0 = _starts(gpr, n, 3)
    out = gpr.device.hmc_chains(lo, hi, X0, np.full(n, np.nan), 3.0 * _factor(gpr, bounds), 0.5, 4, 1.0,
                                gpr.minus_inf_value, 77, 0, steps, 2, hooks=True, reflect=True)
    Xr, yr = out["X"].reshape(-1, d), out["y"].ravel()
    assert out["X"].shape == (n, steps // 2, d)
    np.testing.assert_array_equal(yr, _one_point(gpr, Xr))
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, out["X_last"]))
    assert not np.isnan(out["y_prop"]).any(), "a trajectory was cut short with the cap far away"
    np.testing.assert_array_equal(out["y_prop"].ravel(), _one_point(gpr, out["X_prop"].reshape(-1, d)))
    for k in ("X", "X_last", "X_prop"):
        assert np.all((out[k] >= lo) & (out[k] <= hi)), k
    np.testing.assert_array_equal(out["ncalls"], 1 + steps)
    np.testing.assert_array_equal(out["ngrad"], 1 + 4 * steps)
    assert out["nreflect"].sum() > 0 and out["naccept"].sum() > 0


def test_no_reflecting_state_outside_the_box_or_on_gated_ground_and_only_the_cap_cuts_short():
    gpr, bounds = _svm_model()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n, steps = 32, 25
    X0 = _starts(gpr, n, 5)
    args = (lo, hi, X0, np.full(n, np.nan), 3.0 * _factor(gpr, bounds), 0.5, 4, 1.0, gpr.minus_inf_value, 31, 1, steps, 1)
    out = gpr.device.hmc_chains(*args, hooks=True, reflect=True)
    Xr = out["X"].reshape(-1, 3)
    assert np.all((Xr >= lo) & (Xr <= hi)) and np.all((out["X_prop"] >= lo) & (out["X_prop"] <= hi))
    yr = gpr.predict(Xr)
    assert np.all(np.isfinite(yr)) and np.all(yr > -np.inf)
    np.testing.assert_array_equal(out["y"].ravel(), _one_point(gpr, Xr))
    assert np.any(np.isneginf(out["y_prop"])), "no end point met the gates"
    assert not np.isnan(out["y_prop"]).any() and not np.isnan(out["dH_prop"]).any()
    assert out["nreflect"].sum() > 0 and out["naccept"].sum() > 0
    # the same call without reflection loses trajectories to the box; with max_reflect = 1 and a long step some drifts
    # meet a second wall: those trajectories end there, inside the box, and cost no evaluation
    off = gpr.device.hmc_chains(*args, hooks=True)
    assert np.isnan(off["y_prop"]).sum() > 0
    long = args[:5] + (1.0,) + args[6:]
    one = gpr.device.hmc_chains(*long, hooks=True, reflect=True, max_reflect=1)
    cut = np.isnan(one["y_prop"])
    assert cut.sum() > 0, "max_reflect = 1 never ran out"
    assert np.all((one["X_prop"] >= lo) & (one["X_prop"] <= hi))
    np.testing.assert_array_equal(np.isnan(one["dH_prop"]), cut)
    np.testing.assert_array_equal(one["ncalls"], 1 + np.sum(~cut, axis=1))
    assert np.all(one["ngrad"][cut.any(axis=1)] < 1 + 4 * steps)
    np.testing.assert_array_equal(one["y"].ravel(), _one_point(gpr, one["X"].reshape(-1, 3)))
    many = gpr.device.hmc_chains(*long, hooks=True, reflect=True, max_reflect=1024)
    assert not np.isnan(many["y_prop"]).any()


# ---- determinism ------------------------------------------------------------------------------------------------------
def test_reflecting_chains_same_seed_same_bits_on_two_contexts_any_number_of_chains_and_continued_calls():
    from test_nested_gpu import _fixed, _gauss_ll
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    gpr, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    assert gpr2.device is not gpr.device
    _pushed(gpr), _pushed(gpr2)
    lo, hi = np.full(4, -0.7), np.full(4, 1.3)              # (the mode at 0.3, faces two sigma away)
    inside = np.all((gpr.X_train > lo) & (gpr.X_train < hi), axis=1)
    X0 = np.ascontiguousarray(gpr.X_train[inside][:64])
    assert len(X0) == 64
    Lp = np.linalg.cholesky(np.cov((X0 - lo) / (hi - lo), rowvar=False))
    k = 10
    call = lambda dev, X, y, seed, batch, n: dev.hmc_chains(lo, hi, X, y, Lp, 0.5, 4, 1.0, -np.inf, seed, batch, n, 1,  # noqa: E731
                                                            hooks=True, reflect=True)
    nan = np.full(64, np.nan)
    a = call(gpr.device, X0, nan, 9, 2, 2 * k)
    b = call(gpr2.device, X0, nan, 9, 2, 2 * k)
    e = call(gpr.device, X0[:7], nan[:7], 9, 2, 2 * k)
    for key in KEYS + ("nreflect",):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a[key][:7], e[key], err_msg=key)
    f = call(gpr.device, X0, nan, 10, 2, 2 * k)
    assert not np.array_equal(a["X"], f["X"])
    assert 0 < a["naccept"].sum() < 64 * 2 * k and np.sum(a["nreflect"] > 0) > 32
    assert not np.isnan(a["y_prop"]).any()
    # the first k trajectories of the long call are the short call's, and a call that goes on from X_last / y_last
    # evaluates no start and gives the same bits whichever context goes on
    h1 = call(gpr.device, X0, nan, 9, 2, k)
    for key in ("X", "y", "X_prop", "y_prop", "dH_prop"):
        np.testing.assert_array_equal(a[key][:, :k], h1[key], err_msg=key)
    np.testing.assert_array_equal(h1["X_last"], a["X"][:, k - 1])
    h2 = call(gpr.device, h1["X_last"], h1["y_last"], 9, 3, k)
    np.testing.assert_array_equal(h2["ncalls"], k)
    h3 = call(gpr2.device, h1["X_last"], h1["y_last"], 9, 3, k)
    for key in KEYS + ("nreflect",):
        np.testing.assert_array_equal(h2[key], h3[key], err_msg=key)
    assert h2["nreflect"].sum() > 0


# ---- distribution -----------------------------------------------------------------------------------------------------
def _box_filling_surrogate():
    """Surrogate of N(2.5, 4^2 I) on [-4, 4]^4: a Gaussian as wide as its box with the mode near the corner at hi, from 400
    training points uniform on the box, Matern-5/2 with fixed hyper-parameters (length scales of 3 boxes, as
    test_hmc_gpu._correlated_surrogate)."""
    from test_nested_gpu import make_gpr
    from oracle import gpry_oracle as orc
    d = 4
    rng = np.random.default_rng(21)
    X = rng.uniform(-4, 4, (400, d))
    y = -0.5 * np.sum((X - 2.5) ** 2, axis=1) / 4.0 ** 2
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.log([1e3] + [3.0] * d))
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


@pytest.mark.timeout(900)
def test_run_hmc_with_reflection_agrees_with_run_mcmc_on_a_surrogate_that_fills_its_box():
    from gpry_amd.hmc import run_hmc
    from gpry_amd.mcmc import run_mcmc
    gpr, bounds = _box_filling_surrogate()
    _pushed(gpr)
    nchains, d = 256, 4
    rh = run_hmc(gpr.device, bounds, 5, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value,
                 reflect=True)
    rm = run_mcmc(gpr.device, bounds, 6, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value)
    mh, sh = _chain_means(rh, nchains, d)
    mm, sm = _chain_means(rm, nchains, d)
    se = np.sqrt(sh ** 2 + sm ** 2)
    print(f"reflective HMC: eps = {rh.eps:.3f}, nleap = {rh.nleap}, acceptance = {rh.acceptance:.3f}, {rh.ncalls} + "
          f"{rh.ngrad} evaluations, {rh.nreflect} reflections, {rh.wall_s:.2f} s, R - 1 = {rh.Rminus1[-1]:.4f}; Metropolis: "
          f"acceptance = {rm.acceptance:.3f}, {rm.ncalls} evaluations, {rm.wall_s:.2f} s, R - 1 = {rm.Rminus1[-1]:.4f}; "
          f"max |difference of means| / se = {np.max(np.abs(mh - mm) / se):.2f}")
    assert rh.converged and rm.converged
    assert rh.nreflect > 0
    assert np.all(np.abs(mh - mm) < 5 * se), (mh, mm, se)
    assert 0.5 <= rh.acceptance <= 0.98, rh.acceptance
    assert np.all((rh.X >= bounds[:, 0]) & (rh.X <= bounds[:, 1]))
    np.testing.assert_array_equal(rh.y[:200], _one_point(gpr, rh.X[:200]))


# ---- the public interface ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_mc_sample_from_gp_runs_hmc_with_reflection():
    from gpry_amd._lib import GpryHipError
    from gpry_amd.mc import hmc_settings, mc_sample_from_gp
    from test_mcmc_gpu import _moment_target
    gpr, _, _ = _moment_target("gauss d=2")
    bounds = np.array([[-0.5, 1.1]] * 2)                    # (the target: N(0.3, 0.5^2 I), cut at 1.6 sigma)
    assert hmc_settings(2, {"reflect": True, "max_reflect": 8}) == {"reflect": True, "max_reflect": 8}
    before = gpr.n_eval
    X, y, w = mc_sample_from_gp(gpr, bounds=bounds, sampler="hmc", seed=23, sampler_options={"reflect": True})
    res = mc_sample_from_gp.last_result
    assert res.converged and res.nreflect > 0 and res.ngrad > 0
    assert gpr.n_eval - before == res.ncalls + res.ngrad
    assert X.shape == (len(y), 2) and abs(w.sum() - 1) < 1e-12
    assert np.all((X >= bounds[:, 0]) & (X <= bounds[:, 1]))
    np.testing.assert_array_equal(y[:300], _one_point(gpr, X[:300]))
    # without the option nothing reflects
    mc_sample_from_gp(gpr, bounds=bounds, sampler="hmc", seed=23, sampler_options={"max_batches": 1})
    assert mc_sample_from_gp.last_result.nreflect == 0
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="max_reflect"):
            mc_sample_from_gp(gpr, bounds=bounds, sampler="hmc", seed=23,
                              sampler_options={"reflect": True, "max_reflect": bad})
        with pytest.raises(GpryHipError, match="max_reflect"):
            gpr.device.hmc_chains(bounds[:, 0], bounds[:, 1], np.full((4, 2), 0.3), np.full(4, np.nan), 0.3 * np.eye(2), 0.3,
                                  4, 1.0, -np.inf, 1, 0, 2, 1, reflect=True, max_reflect=bad)
    gpr.device.hmc_chains(bounds[:, 0], bounds[:, 1], np.full((4, 2), 0.3), np.full(4, np.nan), 0.3 * np.eye(2), 0.3, 4,
                          1.0, -np.inf, 1, 0, 2, 1, reflect=True, max_reflect=1024)
