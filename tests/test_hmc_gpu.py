"""The HMC sampler of the surrogate on the device (gpry_amd/csrc/hmc.hip, mean_grad.h + gpry_amd/hmc.py) and the public call
on top of it (gpry_amd/mc.py): the gradient the kernel computes is the one-point predict's, taken to unit-cube coordinates,
at every (DP bucket, kernel id) instantiation; every recorded y equals gpr.predict of its row bit for bit; every
trajectory follows the host reference of tests/tools/hmc_numpy.py on the oracle; no state leaves the box or lies on gated
ground; the same seed gives the same bits on two contexts and whatever the number of chains; run_hmc and run_mcmc agree on
a fitted surrogate; mc_sample_from_gp runs it."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed, _starts
from test_nested_gpu import _one_point, _parity_cases, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hmc_numpy as hn  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

K, S = hn.N_CHAINS, hn.N_TRAJ


def _factor(gpr, bounds):
    """Cholesky factor of the training set's weighted covariance in the unit cube (run_hmc's first mass-matrix inverse)."""
    from gpry_amd.mcmc import _weighted_cov
    from gpry_amd.nested import cholesky_ridged
    span = bounds[:, 1] - bounds[:, 0]
    return cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))


# ---- the gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [100, 1100, 2500])
@pytest.mark.parametrize("d", [2, 5, 9, 17])
@pytest.mark.parametrize("kid", [sw.RBF, sw.M12, sw.M32, sw.M52])
def test_gradient_is_the_one_point_predicts_in_unit_cube_coordinates(kid, d, N):
    """G0 against span x gpr.predict(x[None], return_mean_grad=True), within 1e-7 of its largest entry.  predict's
    gradient is taken in the model's transformed coordinates: for the models with the x-affine map (every other case) the
    raw-coordinate gradient is that over the map's span, here 8."""
    affine = (kid + d + N // 1000) % 2 == 0
    model = sw.Model(d, kid, N, affine=affine, seed=N + d)
    gpr = _pushed(model.gpr())
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)              # (not the model's own box)
    rng = np.random.default_rng(kid + 10 * d)
    X0 = np.ascontiguousarray(np.concatenate([gpr.X_train[rng.choice(N, 8)], rng.uniform(lo, hi, (56, d))]))
    out = gpr.device.hmc_chains(lo, hi, X0, np.full(64, np.nan), np.eye(d), 0.1, 1, 1.0, -np.inf, 1, 0, 0, 1, hooks=True)
    ref = np.array([np.ravel(gpr.predict(x[None, :], return_mean_grad=True)[1]) for x in X0])
    ref = ref * (hi - lo) / (8.0 if affine else 1.0)
    err = np.max(np.abs(out["G0"] - ref))
    print(f"kid={kid} d={d} N={N} affine={affine}: max |G0 - ref| = {err:.3e}, max |ref| = {np.max(np.abs(ref)):.3e}")
    assert np.max(np.abs(ref)) > 0
    assert err <= 1e-7 * np.max(np.abs(ref))
    np.testing.assert_array_equal(out["ngrad"], 1)
    np.testing.assert_array_equal(out["ncalls"], 1)
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, X0))


# ---- recorded y -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_recorded_y_equals_one_point_predict(case):
    gpr, bounds = dict(_parity_cases())[case]()
    _pushed(gpr)
    n, steps = 12, 20
    X0 = _starts(gpr, n, 3)
    out = gpr.device.hmc_chains(bounds[:, 0], bounds[:, 1], X0, np.full(n, np.nan), _factor(gpr, bounds), 0.4, 4, 1.0,
                                gpr.minus_inf_value, 77, 0, steps, 2, hooks=True)
    Xr, yr = out["X"].reshape(-1, len(bounds)), out["y"].ravel()
    assert out["X"].shape == (n, steps // 2, len(bounds))
    np.testing.assert_array_equal(yr, _one_point(gpr, Xr))
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, out["X_last"]))
    ev = ~np.isnan(out["y_prop"].ravel())
    np.testing.assert_array_equal(out["y_prop"].ravel()[ev], _one_point(gpr, out["X_prop"].reshape(-1, len(bounds))[ev]))
    assert np.sum(out["naccept"]) > 0


# ---- the walk ---------------------------------------------------------------------------------------------------------
_WALKS = {}


def _walk(name):
    if name not in _WALKS:
        w = hn.Walk(name)
        _WALKS[name] = (w, w.trace())
    return _WALKS[name]


@pytest.mark.parametrize("name", hn.HMC_CASES)
def test_chain_follows_the_reference_trajectory_by_trajectory(name):
    w, tr = _walk(name)
    gpr = _pushed(w.gpr)
    out = gpr.device.hmc_chains(*w.args(), 1, hooks=True)
    span = w.hi - w.lo
    np.testing.assert_array_equal(out["y"].ravel(), _one_point(gpr, out["X"].reshape(-1, w.model.d)))
    g0 = w.grad_x(w.X0) * span
    assert np.max(np.abs(out["G0"] - g0)) <= 1e-7 * np.max(np.abs(g0))
    X_prev = w.X0
    worst = 0.0
    for s in range(S):
        keep = tr.keep(s)
        where = f"{name}, trajectory {s}: {int(np.sum(~keep))} of {K} chains left out"
        U = (out["X_prop"][:, s] - w.lo) / span
        du = np.max(np.abs(U[keep] - tr.U[s][keep]), initial=0.0)
        worst = max(worst, du)
        print(f"{where}; max |du| = {du:.3e}")
        assert du <= hn.POS_TOL, (where, du)
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
    left = int(np.sum(~keep))
    print(f"{name}: compared {K - left} of {K} chains over {S} trajectories; max |du| = {worst:.3e} "
          f"(tolerance {hn.POS_TOL:.1e}); {int(tr.accepted.sum())} accepted, {int(np.isnan(tr.y).sum())} cut short")
    assert left <= hn.LEFT_OUT_CASE * K, (name, left)


def test_left_out_share_of_the_walk_table():
    left = sum(int(np.sum(~_walk(name)[1].keep(S - 1))) for name in hn.HMC_CASES)
    assert left <= hn.LEFT_OUT_TABLE * K * len(hn.HMC_CASES), left


# ---- box and gates ----------------------------------------------------------------------------------------------------
def test_no_recorded_state_outside_the_box_or_on_gated_ground():
    gpr, bounds = _svm_model()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n, steps = 32, 25
    X0 = _starts(gpr, n, 5)
    out = gpr.device.hmc_chains(lo, hi, X0, np.full(n, np.nan), 3.0 * _factor(gpr, bounds), 0.5, 4, 1.0,
                                gpr.minus_inf_value, 31, 1, steps, 1, hooks=True)
    Xr = out["X"].reshape(-1, 3)
    assert np.all((Xr >= lo) & (Xr <= hi))
    yr = gpr.predict(Xr)
    assert np.all(np.isfinite(yr)) and np.all(yr > -np.inf)
    np.testing.assert_array_equal(out["y"].ravel(), _one_point(gpr, Xr))
    assert np.any(np.isneginf(out["y_prop"])), "no end point met the gates"
    cut = np.isnan(out["y_prop"])
    left = np.any((out["X_prop"] < lo) | (out["X_prop"] > hi), axis=2)
    assert left.sum() > 0, "no trajectory left the box"
    np.testing.assert_array_equal(cut, left)
    np.testing.assert_array_equal(np.isnan(out["dH_prop"]), cut)
    np.testing.assert_array_equal(out["ncalls"], 1 + np.sum(~cut, axis=1))
    assert np.all(out["ngrad"] <= 1 + 4 * steps) and np.all(out["ngrad"][cut.any(axis=1)] < 1 + 4 * steps)
    assert np.sum(out["naccept"]) > 0


# ---- determinism ------------------------------------------------------------------------------------------------------
def test_same_seed_same_bits_on_two_contexts_any_number_of_chains_and_split_calls():
    from test_nested_gpu import _fixed, _gauss_ll
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, theta)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    assert gpr2.device is not gpr.device
    Lp = _factor(_pushed(gpr), bounds)
    _pushed(gpr2)
    X0 = _starts(gpr, 64, 8)
    args = (bounds[:, 0], bounds[:, 1])
    k = 10
    call = lambda dev, X, y, seed, batch, n: dev.hmc_chains(*args, X, y, Lp, 0.4, 4, 1.0, -np.inf, seed, batch, n, 1,  # noqa: E731
                                                            hooks=True)
    nan = np.full(64, np.nan)
    a = call(gpr.device, X0, nan, 9, 2, 2 * k)
    b = call(gpr2.device, X0, nan, 9, 2, 2 * k)
    e = call(gpr.device, X0[:7], nan[:7], 9, 2, 2 * k)
    for key in ("X", "y", "X_last", "y_last", "naccept", "ncalls", "ngrad", "X_prop", "y_prop", "dH_prop", "G0"):
        np.testing.assert_array_equal(a[key], b[key])
        np.testing.assert_array_equal(a[key][:7], e[key])
    f = call(gpr.device, X0, nan, 10, 2, 2 * k)
    assert not np.array_equal(a["X"], f["X"])
    assert 0 < a["naccept"].sum() < 64 * 2 * k
    # Trajectory s of a call draws from (batch, s): a call of 2 k trajectories is not two calls of k with batch and
    # batch + 1 (include/gpry_hip.h).  What holds: the first k trajectories of the long call are the short call's ...
    h1 = call(gpr.device, X0, nan, 9, 2, k)
    for key in ("X", "y", "X_prop", "y_prop", "dH_prop"):
        np.testing.assert_array_equal(a[key][:, :k], h1[key])
    np.testing.assert_array_equal(h1["X_last"], a["X"][:, k - 1])
    # ... and a call that goes on from X_last / y_last evaluates no start and one gradient per chain for it, the same
    # one whichever call goes on
    h2 = call(gpr.device, h1["X_last"], h1["y_last"], 9, 3, k)
    np.testing.assert_array_equal(h2["ncalls"], np.sum(~np.isnan(h2["y_prop"]), axis=1))
    h3 = call(gpr2.device, h1["X_last"], h1["y_last"], 9, 3, k)
    for key in ("X", "y", "X_last", "y_last", "G0", "ngrad"):
        np.testing.assert_array_equal(h2[key], h3[key])
    assert not np.array_equal(h2["X_prop"], a["X_prop"][:, k:])


# ---- distribution -----------------------------------------------------------------------------------------------------
def _correlated_surrogate():
    """Surrogate of N(0.3, C), C_ij = 0.9^|i - j|, d = 8, from 400 training points (half uniform on the box, half around
    the mode), Matern-5/2 with fixed hyper-parameters: length scales of 3 boxes, at which the surrogate follows the
    quadratic within 1 where the mass lies and stays below -20 over the rest of the box."""
    from test_nested_gpu import make_gpr
    from oracle import gpry_oracle as orc
    d = 8
    C = 0.9 ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    P = np.linalg.inv(C)
    rng = np.random.default_rng(17)
    X = np.concatenate([rng.uniform(-4, 4, (200, d)),
                        np.clip(rng.multivariate_normal(np.full(d, 0.3), 2.0 * C, 200), -4.0, 4.0)])
    y = -0.5 * np.einsum("ni,ij,nj->n", X - 0.3, P, X - 0.3)
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.log([1e3] + [3.0] * d))
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


def _chain_means(r, nchains, d):
    Xc = r.X.reshape(nchains, -1, d)
    return r.X.mean(axis=0), Xc.mean(axis=1).std(axis=0, ddof=1) / np.sqrt(nchains)


@pytest.mark.timeout(900)
def test_run_hmc_agrees_with_run_mcmc_on_a_correlated_surrogate():
    from gpry_amd.hmc import run_hmc
    from gpry_amd.mcmc import run_mcmc
    gpr, bounds = _correlated_surrogate()
    _pushed(gpr)
    nchains, d = 256, 8
    rh = run_hmc(gpr.device, bounds, 5, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value)
    rm = run_mcmc(gpr.device, bounds, 6, nchains, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value)
    assert rh.converged and rm.converged
    mh, sh = _chain_means(rh, nchains, d)
    mm, sm = _chain_means(rm, nchains, d)
    se = np.sqrt(sh ** 2 + sm ** 2)
    print(f"HMC: eps = {rh.eps:.3f}, nleap = {rh.nleap}, acceptance = {rh.acceptance:.3f}, {rh.ncalls} + {rh.ngrad} "
          f"evaluations, {rh.wall_s:.2f} s; Metropolis: acceptance = {rm.acceptance:.3f}, {rm.ncalls} evaluations, "
          f"{rm.wall_s:.2f} s; max |difference of means| / se = {np.max(np.abs(mh - mm) / se):.2f}")
    assert np.all(np.abs(mh - mm) < 5 * se), (mh, mm, se)
    assert 0.5 <= rh.acceptance <= 0.98, rh.acceptance
    np.testing.assert_array_equal(rh.y[:200], _one_point(gpr, rh.X[:200]))


# ---- the public interface ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_mc_sample_from_gp_runs_hmc():
    from gpry_amd.mc import hmc_settings, mc_sample_from_gp
    from test_mcmc_gpu import _moment_target
    gpr, bounds, _ = _moment_target("gauss d=2")
    before = gpr.n_eval
    X, y, w = mc_sample_from_gp(gpr, bounds=bounds, sampler="hmc", seed=23)
    res = mc_sample_from_gp.last_result
    assert res.converged and res.ngrad > 0
    assert gpr.n_eval - before == res.ncalls + res.ngrad
    assert X.shape == (len(y), 2) and abs(w.sum() - 1) < 1e-12
    np.testing.assert_array_equal(y[:200], _one_point(gpr, X[:200]))
    assert np.all((X >= bounds[:, 0]) & (X <= bounds[:, 1]))
    # the same sample as the Metropolis chains', within the noise of both
    Xm, _, wm = mc_sample_from_gp(gpr, bounds=bounds, sampler="mcmc", seed=22)
    sd = np.sqrt(wm @ (Xm - wm @ Xm) ** 2)
    assert np.all(np.abs(w @ X - wm @ Xm) < 0.15 * sd), (w @ X, wm @ Xm)
    # an unknown option is refused: warned about and not passed on
    with pytest.warns(UserWarning, match="not recognised"):
        assert hmc_settings(2, {"proposal_scale": 3.0, "nchains": "32d"}) == {"nchains": 64}
    with pytest.warns(UserWarning, match="not recognised"):
        Xs, ys, ws = mc_sample_from_gp(gpr, bounds=bounds, sampler="hmc", seed=23,
                                       sampler_options={"bogus": 1, "max_batches": 1})
    # every row of a (short) sample: y is the one-point predict of its row, bit for bit
    assert 1000 < len(ys) < 20000 and abs(ws.sum() - 1) < 1e-12
    np.testing.assert_array_equal(ys, _one_point(gpr, Xs))
    with pytest.raises(ValueError):
        mc_sample_from_gp(gpr, bounds=bounds, sampler="hamiltonian")


def test_out_of_range_arguments_are_refused_with_a_message():
    from gpry_amd._lib import GpryHipError
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    X0 = _starts(gpr, 4, 1)

    def call(eps=0.3, nleap=4, T=1.0, lo=bounds[:, 0]):
        return gpr.device.hmc_chains(lo, bounds[:, 1], X0, np.full(4, np.nan), np.eye(3), eps, nleap, T, -np.inf, 1, 0, 2, 1)

    call()
    for kw, word in ((dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"), (dict(eps=np.nan), "eps"), (dict(nleap=0), "nleap"),
                     (dict(nleap=1025), "nleap"), (dict(T=0.0), "temperature"), (dict(T=-2.0), "temperature"),
                     (dict(lo=bounds[:, 1]), "bounds")):
        with pytest.raises(GpryHipError, match=word):
            call(**kw)
    call(nleap=1024, eps=1e-3)
