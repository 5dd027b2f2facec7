"""The Metropolis sampler of the surrogate on the device (gpry_amd/csrc/mcmc.hip + gpry_amd/mcmc.py) and the public calls
on top of it (gpry_amd/mc.py, SmallChainProposer): every recorded and proposed y equals gpr.predict of its row bit for bit
(the model cases of test_nested_gpu.py); every step follows the Metropolis rule with the numpy Philox restatement's
draws; the same seed gives the same bits on two contexts and whatever the number of chains in the launch; the moments
of fitted surrogates agree with a quadrature, at T = 1 and, reweighted, at T = 2; mc_sample_from_gp runs both samplers."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_nested_gpu import _banana_ll, _fitted, _gauss_ll, _one_point, _parity_cases, _quadrature

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mcmc_numpy  # noqa: E402,F401
import sampler_walk  # noqa: E402

pytestmark = pytest.mark.gpu


def _pushed(gpr):
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    return gpr


def _proposal(gpr, bounds, scale=1.0):
    from gpry_amd.mcmc import _weighted_cov
    from gpry_amd.nested import cholesky_ridged
    span = bounds[:, 1] - bounds[:, 0]
    d = len(bounds)
    return scale * 2.38 / np.sqrt(d) * cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))


def _starts(gpr, n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(gpr.X_train[rng.choice(len(gpr.X_train), n)])


@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_recorded_and_proposed_y_equals_one_point_predict(case):
    gpr, bounds = dict(_parity_cases())[case]()
    _pushed(gpr)
    n, steps = 12, 40
    X0 = _starts(gpr, n, 3)
    out = gpr.device.mcmc_chains(bounds[:, 0], bounds[:, 1], X0, np.full(n, np.nan), _proposal(gpr, bounds), 1.0,
                                 gpr.minus_inf_value, 77, 0, steps, 2, proposals=True)
    Xr, yr = out["X"].reshape(-1, len(bounds)), out["y"].ravel()
    np.testing.assert_array_equal(yr, _one_point(gpr, Xr))
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, out["X_last"]))
    ev = ~np.isnan(out["y_prop"].ravel())
    Xp = out["X_prop"].reshape(-1, len(bounds))[ev]
    np.testing.assert_array_equal(out["y_prop"].ravel()[ev], _one_point(gpr, Xp))
    assert np.all(np.isfinite(yr)) and np.all((Xr >= bounds[:, 0]) & (Xr <= bounds[:, 1]))
    # the start's evaluation and one per evaluated proposal
    np.testing.assert_array_equal(out["ncalls"], 1 + np.sum(~np.isnan(out["y_prop"]), axis=1))
    assert np.sum(out["naccept"]) > 0
    if case == "SVM + trust region":
        assert np.any(np.isneginf(out["y_prop"])), "no proposal met the gates"
        assert np.all(gpr.predict(Xr) > -np.inf)


@pytest.mark.parametrize("scale,T", [(1.0, 1.0), (6.0, 1.5)])
def test_every_step_follows_the_metropolis_rule(scale, T):
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    n, steps, seed, batch = 16, 60, 1234, 5
    Lp = _proposal(gpr, bounds, scale)
    X0 = _starts(gpr, n, 4)
    # (the body of the check: tests/tools/sampler_walk.py, which test_sampler_walk_gpu.py runs at every instantiation)
    counts = sampler_walk.check_metropolis_rule(gpr.device, lo, hi, X0, np.full(n, np.nan), _one_point(gpr, X0), Lp, T,
                                                gpr.minus_inf_value, seed, batch, steps, 1)
    outside = counts["outside"]
    if scale > 1:
        assert outside > 0, "the wide proposal never left the box"


def test_same_seed_same_bits_on_two_contexts_and_any_number_of_chains():
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    from test_nested_gpu import _fixed
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, theta)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    assert gpr2.device is not gpr.device
    Lp = _proposal(_pushed(gpr), bounds)
    _pushed(gpr2)
    X0 = _starts(gpr, 64, 8)
    args = (bounds[:, 0], bounds[:, 1])
    a = gpr.device.mcmc_chains(*args, X0, np.full(64, np.nan), Lp, 1.0, -np.inf, 9, 2, 50, 1)
    b = gpr2.device.mcmc_chains(*args, X0, np.full(64, np.nan), Lp, 1.0, -np.inf, 9, 2, 50, 1)
    e = gpr.device.mcmc_chains(*args, X0[:8], np.full(8, np.nan), Lp, 1.0, -np.inf, 9, 2, 50, 1)
    for k in ("X", "y", "X_last", "y_last", "naccept", "ncalls"):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][:8], e[k])
    f = gpr.device.mcmc_chains(*args, X0, np.full(64, np.nan), Lp, 1.0, -np.inf, 10, 2, 50, 1)
    assert not np.array_equal(a["X"], f["X"])


def _moment_target(target):
    if target == "gauss d=2":
        gpr, bounds = _fitted(_gauss_ll(2), 2, 200)
        return gpr, bounds, 400
    if target == "gauss d=4":
        gpr, bounds = _fitted(_gauss_ll(4), 4, 400)
        return gpr, bounds, 40
    gpr, bounds = _fitted(_banana_ll, 2, 300)
    return gpr, bounds, 400


def _moments(X, w):
    m = w @ X
    return m, (X - m).T @ ((X - m) * w[:, None])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("target", ["gauss d=2", "gauss d=4", "banana d=2"])
def test_moments_against_quadrature(target):
    from gpry_amd.mcmc import run_mcmc
    gpr, bounds, n = _moment_target(target)
    _, mq, Cq = _quadrature(gpr, bounds, n)
    sd = np.sqrt(np.diag(Cq))
    _pushed(gpr)
    for seed in (1, 2, 3):
        r = run_mcmc(gpr.device, bounds, seed, 256, gpr.X_train, gpr.y_train, minus_inf_value=gpr.minus_inf_value)
        assert r.converged and r.Rminus1[-1] < 0.01, (seed, r.Rminus1[-5:])
        assert 0.05 < r.acceptance < 0.9, r.acceptance
        m, C = _moments(r.X, r.w)
        assert np.all(np.abs(m - mq) < 0.1 * sd), (seed, m, mq, sd)
        assert np.all(np.abs(C - Cq) <= 0.2 * np.outer(sd, sd)), (seed, C, Cq)
        np.testing.assert_array_equal(r.y[:200], _one_point(gpr, r.X[:200]))


@pytest.mark.timeout(900)
def test_temperature_two_is_reweighted_to_one():
    from gpry_amd.mcmc import run_mcmc
    gpr, bounds, n = _moment_target("gauss d=2")
    _, mq, Cq = _quadrature(gpr, bounds, n)
    sd = np.sqrt(np.diag(Cq))
    _pushed(gpr)
    r = run_mcmc(gpr.device, bounds, 4, 256, gpr.X_train, gpr.y_train, temperature=2.0,
                 minus_inf_value=gpr.minus_inf_value)
    assert r.converged
    _, Cu = _moments(r.X, np.full(len(r.y), 1.0 / len(r.y)))
    assert np.all(np.abs(Cu - 2 * Cq) <= 0.4 * np.outer(sd, sd)), (Cu, 2 * Cq)
    m, C = _moments(r.X, r.w)
    assert np.all(np.abs(m - mq) < 0.1 * sd), (m, mq)
    assert np.all(np.abs(C - Cq) <= 0.2 * np.outer(sd, sd)), (C, Cq)


@pytest.mark.timeout(900)
def test_mc_sample_from_gp_runs_both_samplers(tmp_path):
    from gpry_amd.mc import mc_sample_from_gp
    from gpry_amd.nested import run_nested
    gpr, bounds, _ = _moment_target("gauss d=2")
    opts = {"nlive": "250d", "num_repeats": "5d", "precision_criterion": 0.01, "nprior": 5000}
    X, y, w = mc_sample_from_gp(gpr, bounds=bounds, sampler="nested", sampler_options=opts, seed=21,
                                output=str(tmp_path / "ns"))
    r = run_nested(gpr.device, bounds, 21, 500, 10, precision_criterion=0.01, nprior=5000,
                   minus_inf_value=gpr.minus_inf_value)
    np.testing.assert_array_equal(X, r.X)
    np.testing.assert_array_equal(y, r.y)
    np.testing.assert_array_equal(w, r.w)
    table = np.loadtxt(tmp_path / "ns.txt")
    np.testing.assert_allclose(table[:, 1], -y, rtol=1e-15)
    Xm, ym, wm = mc_sample_from_gp(gpr, bounds=bounds, sampler="mcmc", seed=22)
    assert mc_sample_from_gp.last_result.converged
    m, C = _moments(X, w)
    mm, Cm = _moments(Xm, wm)
    sd = np.sqrt(np.diag(C))
    assert np.all(np.abs(m - mm) < 0.15 * sd), (m, mm)
    assert np.all(np.abs(C - Cm) <= 0.3 * np.outer(sd, sd)), (C, Cm)
    np.testing.assert_array_equal(ym[:200], _one_point(gpr, Xm[:200]))
    # the default bounds are the model's
    Xd, _, _ = mc_sample_from_gp(gpr, sampler="mcmc", seed=22, sampler_options={"max_samples": 20000})
    assert np.all((Xd >= gpr.bounds[:, 0]) & (Xd <= gpr.bounds[:, 1]))


def test_small_chain_proposer():
    from gpry_amd.gp_acquisition import BatchOptimizer
    from gpry_amd.proposal import SmallChainProposer
    gpr, bounds, _ = _moment_target("gauss d=2")
    p = SmallChainProposer(bounds, npoints=100, nsteps=20)
    p.update(gpr)
    rng = np.random.default_rng(3)
    pts = np.array([p.get(rng=rng) for _ in range(5)])
    assert np.all((pts >= bounds[:, 0]) & (pts <= bounds[:, 1]))
    # the same chain again: a training point drawn by rng.choice, then the device chain seeded from the rng
    rng = np.random.default_rng(3)
    i = rng.choice(range(len(gpr.X_train)))
    seed = int(rng.integers(2**31 - 1))
    from gpry_amd.mcmc import _weighted_cov
    from gpry_amd.nested import cholesky_ridged
    span = bounds[:, 1] - bounds[:, 0]
    Lp = 2.38 / np.sqrt(2) * cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))
    out = gpr.device.mcmc_chains(bounds[:, 0], bounds[:, 1], gpr.X_train[i:i + 1], np.array([np.nan]), Lp, 1.0,
                                 gpr.minus_inf_value, seed, 0, 100, 1)
    kept = out["X"][0][::-20]
    np.testing.assert_array_equal(pts, kept[::-1][:5])
    acq = BatchOptimizer(bounds, proposer=SmallChainProposer(bounds, npoints=60, nsteps=10), n_restarts_optimizer=2,
                         n_repeats_propose=1, verbose=0)
    Xo, yl, av = acq.multi_add(gpr, n_points=2, rng=np.random.default_rng(5))
    assert Xo.shape == (2, 2) and np.all(np.isfinite(av))
    assert np.all((Xo >= bounds[:, 0]) & (Xo <= bounds[:, 1]))
