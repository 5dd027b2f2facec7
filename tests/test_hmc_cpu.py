"""The HMC sampler without a GPU: the numpy stand-in of the device call (tests/tools/hmc_numpy.py) under the host loop of
gpry_amd/hmc.py, and what tests/test_hmc_gpu.py relies on: leapfrog is reversible; the same seed gives the same bits,
whatever the number of chains; no state leaves the box and a trajectory that does costs no evaluation; run_hmc recovers a
correlated Gaussian; the float64 restatement's noise floor (against long double) is below the EPS_H the GPU position
tolerance is made from, and its margins leave out few enough chains of the walk table."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hmc_numpy as hn  # noqa: E402

K, S = hn.N_CHAINS, hn.N_TRAJ


def _gauss(d, rho=0.9, mu=0.3):
    """Log-density and gradient of N(mu, C), C_ij = rho^|i - j| (correlation rho between neighbours)."""
    C = rho ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    P = np.linalg.inv(C)
    ll = lambda X: -0.5 * np.einsum("ni,ij,nj->n", np.atleast_2d(X) - mu, P, np.atleast_2d(X) - mu)      # noqa: E731
    gr = lambda X: -(np.atleast_2d(X) - mu) @ P                                                          # noqa: E731
    return C, ll, gr


def test_leapfrog_followed_by_a_momentum_flip_is_an_involution():
    d, n = 8, 32
    C, ll, gr = _gauss(d)
    lo, span = np.full(d, -8.0), np.full(d, 16.0)
    rng = np.random.default_rng(0)
    u0 = (rng.multivariate_normal(np.full(d, 0.3), C, n) - lo) / span
    p0 = rng.normal(size=(n, d))
    Lp = np.linalg.cholesky(C / np.outer(span, span))
    eps = np.full(n, 0.3)
    grad_u = lambda X: gr(X) * span          # noqa: E731
    u1, x1, g1, p1, alive, _, ng = hn.leapfrog(grad_u, lo, span, u0, grad_u(lo + u0 * span), p0, Lp, eps, 7, 1.0)
    assert alive.all() and np.all(ng == 7) and np.max(np.abs(u1 - u0)) > 1e-3
    u2, _, _, p2, alive2, _, _ = hn.leapfrog(grad_u, lo, span, u1, g1, -p1, Lp, eps, 7, 1.0)
    assert alive2.all()
    assert np.max(np.abs(u2 - u0)) < 1e-10 and np.max(np.abs(p2 + p0)) < 1e-10
    # and the energy error of the trajectory is that of a second-order integrator
    H = lambda u, p: -ll(lo + u * span) + 0.5 * np.sum(p * p, axis=1)      # noqa: E731
    assert np.max(np.abs(H(u1, p1) - H(u0, p0))) < 0.5


def _call(dev, X0, seed=5, nsteps=12, eps=0.3, nleap=4, T=1.0, d=4, half=6.0, **kw):
    lo, hi = np.full(d, -half), np.full(d, half)
    Lp = np.linalg.cholesky(_gauss(d)[0] / (2 * half) ** 2)
    return dev.hmc_chains(lo, hi, X0, np.full(len(X0), np.nan), Lp, eps, nleap, T, -np.inf, seed, 2, nsteps, 1, hooks=True,
                          **kw)


def test_same_seed_same_bits_and_any_number_of_chains():
    d = 4
    C, ll, gr = _gauss(d)
    X0 = np.random.default_rng(1).multivariate_normal(np.full(d, 0.3), C, 64)
    a, b = _call(hn.HmcNumpyDevice(ll, gr), X0), _call(hn.HmcNumpyDevice(ll, gr), X0)
    e = _call(hn.HmcNumpyDevice(ll, gr), X0[:7])
    f = _call(hn.HmcNumpyDevice(ll, gr), X0, seed=6)
    for k in ("X", "y", "X_last", "y_last", "naccept", "ncalls", "ngrad", "X_prop", "y_prop", "dH_prop", "G0"):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][:7], e[k])
    assert not np.array_equal(a["X"], f["X"])
    assert 0 < a["naccept"].sum() < a["naccept"].size * 12


def test_no_state_leaves_the_box_and_a_trajectory_that_does_costs_no_evaluation():
    d, n, nsteps = 4, 48, 20
    C, ll, gr = _gauss(d)
    rng = np.random.default_rng(2)
    lo, hi = np.full(d, -1.5), np.full(d, 1.5)          # (faces 1.5 sigma from the mode: the gradient there is mild)
    U0 = rng.uniform(0.3, 0.7, (n, d))
    face = rng.integers(0, d, n)
    U0[np.arange(n), face] = np.where(rng.random(n) < 0.5, rng.uniform(0, 1e-3, n), 1 - rng.uniform(0, 1e-3, n))
    X0 = lo + U0 * (hi - lo)
    out = _call(hn.HmcNumpyDevice(ll, gr), X0, nsteps=nsteps, eps=0.5, half=1.5)
    assert np.all((out["X"] >= lo) & (out["X"] <= hi)) and np.all((out["X_last"] >= lo) & (out["X_last"] <= hi))
    left = np.any((out["X_prop"] < lo) | (out["X_prop"] > hi), axis=2)
    assert left.sum() > 10, "no trajectory left the box"
    assert np.all(np.isnan(out["y_prop"][left])) and np.all(np.isnan(out["dH_prop"][left]))
    np.testing.assert_array_equal(out["ncalls"], 1 + np.sum(~np.isnan(out["y_prop"]), axis=1))
    assert np.all(out["ngrad"] <= 1 + 4 * nsteps) and np.all(out["ngrad"][left.any(axis=1)] < 1 + 4 * nsteps)


def test_run_hmc_recovers_a_correlated_gaussian():
    from gpry_amd.hmc import run_hmc
    d, nchains = 8, 64
    C, ll, gr = _gauss(d)
    bounds = np.array([[-8.0, 8.0]] * d)
    Xt = np.random.default_rng(3).multivariate_normal(np.full(d, 0.3), 1.5 * C, 400)
    dev = hn.HmcNumpyDevice(ll, gr)
    r = run_hmc(dev, bounds, 11, nchains, Xt, ll(Xt))
    assert r.converged and r.Rminus1[-1] < 0.01
    assert 0.5 < r.acceptance < 0.99, r.acceptance
    assert r.nleap == int(np.clip(np.ceil(1.57 / r.eps), 4, 64))
    frozen = [c for c in dev.calls[6:]]
    assert all(c["eps"] == r.eps and c["nleap"] == r.nleap and np.array_equal(c["Lp"], frozen[0]["Lp"]) for c in frozen)
    assert [c["batch"] for c in dev.calls] == list(range(len(dev.calls)))
    assert abs(r.w.sum() - 1) < 1e-12 and r.ngrad > r.ncalls
    Xc = r.X.reshape(nchains, -1, d)
    se = Xc.mean(axis=1).std(axis=0, ddof=1) / np.sqrt(nchains)
    m = r.X.mean(axis=0)
    print(f"eps = {r.eps:.3f}, nleap = {r.nleap}, acceptance = {r.acceptance:.3f}, {len(r.X)} rows, "
          f"max |mean - mu| / se = {np.max(np.abs(m - 0.3) / se):.2f}, "
          f"variance ratios {np.min(r.X.var(axis=0) / np.diag(C)):.3f} .. {np.max(r.X.var(axis=0) / np.diag(C)):.3f}")
    assert np.all(np.abs(m - 0.3) < 5 * se), (m, se)
    assert np.all(np.abs(r.X.var(axis=0) / np.diag(C) - 1) < 0.15), r.X.var(axis=0)


def test_run_hmc_tempered_is_reweighted():
    from gpry_amd.hmc import run_hmc
    d = 3
    C, ll, gr = _gauss(d)
    bounds = np.array([[-10.0, 10.0]] * d)
    Xt = np.random.default_rng(4).multivariate_normal(np.full(d, 0.3), 2 * C, 300)
    r = run_hmc(hn.HmcNumpyDevice(ll, gr), bounds, 12, 64, Xt, ll(Xt), temperature=2.0)
    assert r.converged
    var_flat = r.X.var(axis=0)
    m = r.w @ r.X
    var_w = r.w @ (r.X - m) ** 2
    assert np.all(np.abs(var_flat / 2 - 1) < 0.2), var_flat
    assert np.all(np.abs(var_w - 1) < 0.2), var_w


# ---- the walk table ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    out = {}
    for name in hn.HMC_CASES:
        w = hn.Walk(name, gpr_device=OracleDevice())
        out[name] = dict(w=w, tr=w.trace(), ld=w.trace(dtype=np.longdouble))
    return out


def test_the_table_has_the_cases_the_walk_test_is_set():
    import sampler_walk as sw
    models = [hn._cases()[n][0] for n in hn.HMC_CASES]
    plain = {(m["kid"], m["d"], m["N"]) for m in models if not m.get("svm")}
    assert plain >= {(kid, d, N) for kid in range(4) for d in (3, 16) for N in (100, 1100)}
    assert {sw.dp_bucket(m["d"]) for m in models} >= {4, 16}
    assert {m.get("affine", True) for m in models} == {True, False}
    assert any(m.get("svm") for m in models) and any(T != 1.0 for _, T in hn._cases().values())
    assert (hn.N_CHAINS, hn.N_TRAJ, hn.N_LEAP) == (64, 8, 5)


def test_noise_floor_and_left_out_shares(table):
    eps_h, total, accepted, cut = 0.0, 0, 0, 0
    for name, e in table.items():
        tr, ld = e["tr"], e["ld"]
        for s in range(S):
            both = tr.keep(s) & ld.keep(s)
            # the same decisions in both precisions for the chains the margins keep
            np.testing.assert_array_equal(tr.accepted[s][both], ld.accepted[s][both], err_msg=name)
            np.testing.assert_array_equal(tr.ncalls[s][both], ld.ncalls[s][both], err_msg=name)
            eps_h = max(eps_h, float(np.max(np.abs(tr.U[s][both] - ld.U[s][both]), initial=0.0)))
        left = int(np.sum(~(tr.keep(S - 1) & ld.keep(S - 1))))
        total += left
        accepted += int(tr.accepted.sum())
        cut += int(np.isnan(tr.y).sum())
        print(f"{name}: {left} of {K} chains left out, {int(tr.accepted.sum())} of {K * S} trajectories accepted, "
              f"{int(np.isnan(tr.y).sum())} cut short")
        assert left <= hn.LEFT_OUT_CASE * K, (name, left)
    print(f"eps_h = {eps_h:.3g} (EPS_H = {hn.EPS_H:g}); {total} of {K * len(table)} chains left out")
    assert total <= hn.LEFT_OUT_TABLE * K * len(table), total
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:      # (where long double is wider than double)
        assert 0.0 < eps_h <= hn.EPS_H, eps_h
    assert hn.POS_TOL == 100 * hn.EPS_H
    # the table exercises both outcomes and the early rejection
    assert accepted > 0.2 * K * S * len(table) and cut > 0


def test_the_gated_case_meets_the_gates(table):
    tr = table["gated"]["tr"]
    assert np.sum(np.isneginf(tr.y)) > 0, "no end point met the gates"
    assert not np.any(tr.accepted & np.isneginf(tr.y))
