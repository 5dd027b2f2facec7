"""Reflective HMC without a GPU: the numpy restatement of the reflective drift (tests/tools/hmc_reflect_numpy.py) under
the host loop of gpry_amd/hmc.py, and what tests/test_hmc_reflect_gpu.py relies on: the reflective leapfrog followed by a
momentum flip is an involution and a drift keeps |p|^2; with reflection off the stand-in is hmc_numpy's bit for bit, and so
it is with reflection on in a box no chain touches; with reflection no state leaves the box and no trajectory is lost to
it, short of the cap; the walk table meets the conditions the GPU walk test is set; run_hmc(reflect=True) recovers a
uniform and a truncated Gaussian target that fill their box."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hmc_numpy as hn  # noqa: E402
import hmc_reflect_numpy as hr  # noqa: E402

K, S = hr.N_CHAINS, hr.N_TRAJ
KEYS = ("X", "y", "X_last", "y_last", "naccept", "ncalls", "ngrad", "X_prop", "y_prop", "dH_prop", "G0")


def _gauss(d, rho=0.9, mu=0.3):
    """Log-density and gradient of N(mu, C), C_ij = rho^|i - j| (tests/test_hmc_cpu.py: _gauss)."""
    C = rho ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    P = np.linalg.inv(C)
    ll = lambda X: -0.5 * np.einsum("ni,ij,nj->n", np.atleast_2d(X) - mu, P, np.atleast_2d(X) - mu)      # noqa: E731
    gr = lambda X: -(np.atleast_2d(X) - mu) @ P                                                          # noqa: E731
    return C, ll, gr


def _call(dev, X0, half, seed=5, nsteps=12, eps=0.3, nleap=4, d=4, **kw):
    lo, hi = np.full(d, -half), np.full(d, half)
    Lp = np.linalg.cholesky(_gauss(d)[0] / (2 * half) ** 2)
    return dev.hmc_chains(lo, hi, X0, np.full(len(X0), np.nan), Lp, eps, nleap, 1.0, -np.inf, seed, 2, nsteps, 1, hooks=True,
                          **kw)


def _chain_means(r, nchains, d):
    from test_hmc_gpu import _chain_means as f
    return f(r, nchains, d)


# ---- the map ----------------------------------------------------------------------------------------------------------
def test_reflective_leapfrog_then_momentum_flip_is_an_involution_and_a_drift_keeps_the_kinetic_energy():
    d, n = 6, 256
    C, ll, gr = _gauss(d)
    lo, span = np.full(d, -1.2), np.full(d, 2.4)          # (faces about one sigma from the mode)
    rng = np.random.default_rng(0)
    u0 = rng.uniform(0.02, 0.98, (n, d))
    p0 = rng.normal(size=(n, d))
    Lp = np.linalg.cholesky(C / np.outer(span, span))
    eps = np.full(n, 0.3)
    grad_u = lambda X: gr(X) * span          # noqa: E731
    u1, x1, g1, p1, alive, st, ng = hr.leapfrog(grad_u, lo, span, u0, grad_u(lo + u0 * span), p0, Lp, eps, 7, 1.0)
    assert alive.all() and np.all(ng == 7)
    refl = st["nrefl"] > 0
    assert refl.sum() > n // 2 and np.sum(st["maxdrift"] >= 2) > 5, (refl.sum(), st["maxdrift"].max())
    assert np.all((u1 >= 0) & (u1 <= 1))
    u2, _, _, p2, alive2, st2, _ = hr.leapfrog(grad_u, lo, span, u1, g1, -p1, Lp, eps, 7, 1.0)
    assert alive2.all()
    np.testing.assert_array_equal(st2["nrefl"][refl], st["nrefl"][refl])
    print(f"{int(refl.sum())} of {n} trajectories reflect, up to {st['maxdrift'].max()} times in a drift; "
          f"max |u2 - u0| = {np.max(np.abs(u2 - u0)[refl]):.2e}, max |p2 + p0| = {np.max(np.abs(p2 + p0)[refl]):.2e}, "
          f"max change of |p|^2 over a drift = {max(st['dp2'].max(), st2['dp2'].max()):.2e}")
    assert np.max(np.abs(u2 - u0)[refl]) < 1e-10 and np.max(np.abs(p2 + p0)[refl]) < 1e-10
    # |p|^2 across every drift: to the rounding of the reflections (|p|^2 is of order d)
    assert max(st["dp2"].max(), st2["dp2"].max()) < 1e-12
    # and the reflection is the specular one: the velocity's component along the wall's coordinate flips
    u, p = np.array([[0.5, 0.99]]), np.array([[0.3, 1.0]])
    L = np.linalg.cholesky(np.array([[1.0, 0.6], [0.6, 1.0]]))
    v0 = p @ L.T
    hr.billiard(u, p, L, np.array([0.02]), np.array([True]), 4)
    v1 = p @ L.T
    q0, q1 = np.linalg.solve(L, v0[0]), np.linalg.solve(L, v1[0])       # (whitened velocities: p itself)
    assert abs(v1[0, 1] + v0[0, 1]) < 1e-15 and abs(q1 @ q1 - q0 @ q0) < 1e-15 and 0 <= u[0, 1] < 1
    # the component of the whitened velocity in the wall's plane (orthogonal to row 1 of L) is kept
    t = np.array([L[1, 1], -L[1, 0]])
    assert abs(t @ q1 - t @ q0) < 1e-15


# ---- the stand-in -----------------------------------------------------------------------------------------------------
def test_reflect_off_is_hmc_numpy_bit_for_bit():
    d = 4
    C, ll, gr = _gauss(d)
    X0 = np.random.default_rng(1).multivariate_normal(np.full(d, 0.3), C, 48)
    for half in (6.0, 1.5):                     # (nothing leaves the box; trajectories are cut short by it)
        X = np.clip(X0, -half + 1e-3, half - 1e-3)
        a, b = _call(hn.HmcNumpyDevice(ll, gr), X, half), _call(hr.HmcReflectNumpyDevice(ll, gr), X, half)
        assert "nreflect" not in b
        for k in KEYS:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.isnan(a["y_prop"]).sum() > 0


def test_reflect_on_in_a_box_no_chain_touches_is_reflect_off_bit_for_bit():
    d = 4
    C, ll, gr = _gauss(d)
    X0 = np.random.default_rng(1).multivariate_normal(np.full(d, 0.3), C, 48)
    a = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 9.0)
    b = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 9.0, reflect=True)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(b["nreflect"], 0)
    assert 0 < a["naccept"].sum() < a["naccept"].size * 12


def test_no_state_leaves_the_box_and_only_the_cap_cuts_a_trajectory_short():
    d, n, nsteps = 4, 48, 20
    C, ll, gr = _gauss(d)
    rng = np.random.default_rng(2)
    lo, hi = np.full(d, -1.5), np.full(d, 1.5)
    U0 = rng.uniform(0.3, 0.7, (n, d))
    face = rng.integers(0, d, n)
    U0[np.arange(n), face] = np.where(rng.random(n) < 0.5, rng.uniform(0, 1e-3, n), 1 - rng.uniform(0, 1e-3, n))
    X0 = lo + U0 * (hi - lo)
    kw = dict(nsteps=nsteps, eps=0.5)
    off = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 1.5, **kw)
    assert np.isnan(off["y_prop"]).sum() > 10, "without reflection no trajectory left the box"
    out = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 1.5, reflect=True, **kw)
    for k in ("X", "X_last", "X_prop"):
        assert np.all((out[k] >= lo) & (out[k] <= hi)), k
    assert not np.isnan(out["y_prop"]).any() and not np.isnan(out["dH_prop"]).any()
    np.testing.assert_array_equal(out["ncalls"], 1 + nsteps)
    np.testing.assert_array_equal(out["ngrad"], 1 + 4 * nsteps)
    assert np.all(out["nreflect"] > 0) and 0 < out["naccept"].sum()
    # max_reflect = 1: a drift that meets a second wall ends the trajectory, unevaluated
    L3 = dict(kw, eps=1.5)
    one = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 1.5, reflect=True, max_reflect=1, **L3)
    cut = np.isnan(one["y_prop"])
    assert cut.sum() > 10, cut.sum()
    assert np.all(np.isnan(one["dH_prop"][cut]))
    np.testing.assert_array_equal(one["ncalls"], 1 + np.sum(~cut, axis=1))
    assert np.all(one["ngrad"][cut.any(axis=1)] < 1 + 4 * nsteps)
    for k in ("X", "X_last", "X_prop"):
        assert np.all((one[k] >= lo) & (one[k] <= hi)), k
    many = _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 1.5, reflect=True, **L3)
    assert not np.isnan(many["y_prop"]).any()
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="max_reflect"):
            _call(hr.HmcReflectNumpyDevice(ll, gr), X0, 1.5, reflect=True, max_reflect=bad)


# ---- the walk table ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    out = {}
    for name in hr.REFLECT_CASES:
        w = hr.Walk(name, gpr_device=OracleDevice())
        out[name] = dict(w=w, tr=w.trace(), ld=w.trace(dtype=np.longdouble))
    return out


def test_the_table_has_the_cases_the_walk_test_is_set():
    import sampler_walk as sw
    cases = hr._cases()
    models = [cases[n][0] for n in hr.REFLECT_CASES]
    plain = {(m["kid"], m["d"]) for m in models if not m.get("svm")}
    assert plain >= {(kid, d) for kid in (sw.RBF, sw.M52) for d in (2, 5, 16, 32)}
    assert {sw.dp_bucket(m["d"]) for m in models} == {4, 8, 16, 32}
    for kid in (sw.RBF, sw.M52):
        assert {m["N"] for m in models if m["kid"] == kid and m["d"] in (2, 5, 16, 32) and not m.get("svm")} >= {100, 1100}
    assert any(m.get("svm") for m in models) and any(T != 1.0 for _, T, _ in cases.values())
    assert "corner" in cases and (hr.N_CHAINS, hr.N_TRAJ, hr.N_LEAP) == (64, 8, 5)


def test_every_call_has_a_box_narrower_than_the_models_with_walls_near_the_starts(table):
    for name, e in table.items():
        w = e["w"]
        assert np.all(w.lo > w.model.bounds[:, 0]) and np.all(w.hi < w.model.bounds[:, 1])
        assert np.all((w.X0 > w.lo) & (w.X0 < w.hi))
        sd = w.X0.std(axis=0)
        near = np.minimum(np.min(w.X0 - w.lo, axis=0), np.min(w.hi - w.X0, axis=0))
        assert np.all(near < sd), (name, near / sd)           # (a wall within one standard deviation of some start)


def test_noise_floor_left_out_shares_and_reflections_of_the_table(table):
    eps_h, total = 0.0, 0
    for name, e in table.items():
        tr, ld = e["tr"], e["ld"]
        for s in range(S):
            both = tr.keep(s) & ld.keep(s)
            np.testing.assert_array_equal(tr.accepted[s][both], ld.accepted[s][both], err_msg=name)
            np.testing.assert_array_equal(tr.ncalls[s][both], ld.ncalls[s][both], err_msg=name)
            np.testing.assert_array_equal(tr.nreflect[s][both], ld.nreflect[s][both], err_msg=name)
            eps_h = max(eps_h, float(np.max(np.abs(tr.U[s][both] - ld.U[s][both]), initial=0.0)))
        left = int(np.sum(~(tr.keep(S - 1) & ld.keep(S - 1))))
        total += left
        share = float(np.mean(tr.nrefl > 0))
        print(f"{name}: {left} of {K} chains left out, {share:.2f} of the trajectories reflect, up to "
              f"{int(tr.maxdrift.max())} times in a drift ({int(np.sum(tr.maxdrift >= 2))} trajectories with a drift of two "
              f"or more), {int(tr.accepted.sum())} of {K * S} accepted, {int(np.isnan(tr.y).sum())} cut short")
        assert left <= hr.LEFT_OUT_CASE * K, (name, left)
        assert share >= 0.30, (name, share)
        assert np.all((tr.U >= 0) & (tr.U <= 1)) and np.all((tr.X >= e["w"].lo) & (tr.X <= e["w"].hi)), name
        assert not np.isnan(tr.y).any(), name                       # (nothing is cut short: the cap is far)
        assert tr.margin_cap.min() >= hr.MAX_REFLECT - tr.maxdrift.max() > 0, name
        assert 0.2 * K * S < tr.accepted.sum() < K * S, name
    print(f"eps_h = {eps_h:.3g} (EPS_H = {hr.EPS_H:g}); {total} of {K * len(table)} chains left out")
    assert total <= hr.LEFT_OUT_TABLE * K * len(table), total
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:      # (where long double is wider than double)
        assert 0.0 < eps_h <= hr.EPS_H, eps_h
    assert hr.POS_TOL == 100 * hr.EPS_H and hr.POS_TOL < hr.MARGIN
    assert np.sum(table["corner"]["tr"].maxdrift >= 2) > 20
    trg = table["gated"]["tr"]
    assert np.sum(np.isneginf(trg.y)) > 0 and not np.any(trg.accepted & np.isneginf(trg.y))


# ---- the run loop on targets that fill their box ----------------------------------------------------------------------
def test_run_hmc_with_reflection_recovers_the_uniform_distribution():
    from gpry_amd.hmc import run_hmc
    d, nchains = 3, 64
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 5.0, 2.5])
    bounds = np.stack([lo, hi], axis=1)
    ll = lambda X: np.zeros(len(np.atleast_2d(X)))              # noqa: E731
    gr = lambda X: np.zeros_like(np.atleast_2d(X))              # noqa: E731
    Xt = np.random.default_rng(3).uniform(lo, hi, (300, d))
    dev = hr.HmcReflectNumpyDevice(ll, gr)
    r = run_hmc(dev, bounds, 11, nchains, Xt, ll(Xt), reflect=True)
    assert r.converged and r.nreflect > 0 and r.acceptance > 0.999
    assert all(c["reflect"] and c["max_reflect"] == 64 for c in dev.calls)
    U = (r.X - lo) / (hi - lo)
    ru = r._replace(X=U)
    m, se = _chain_means(ru, nchains, d)
    v, sev = _chain_means(ru._replace(X=(U - 0.5) ** 2), nchains, d)
    print(f"uniform: eps = {r.eps:.3f}, nleap = {r.nleap}, {len(r.X)} rows, {r.nreflect} reflections; "
          f"max |mean - 1/2| / se = {np.max(np.abs(m - 0.5) / se):.2f}, max |var - 1/12| / se = "
          f"{np.max(np.abs(v - 1 / 12) / sev):.2f}")
    assert np.all((U >= 0) & (U <= 1))
    assert np.all(np.abs(m - 0.5) < 5 * se), (m, se)
    assert np.all(np.abs(v - 1.0 / 12.0) < 5 * sev), (v, sev)
    # reflection off on the same target loses trajectories to the walls
    off = run_hmc(hr.HmcReflectNumpyDevice(ll, gr), bounds, 11, nchains, Xt, ll(Xt), max_batches=2)
    assert off.nreflect == 0 and off.acceptance < 0.9


def test_run_hmc_with_reflection_recovers_a_truncated_gaussian():
    from scipy.stats import truncnorm
    from gpry_amd.hmc import run_hmc
    d, nchains = 4, 64
    sig = np.array([0.5, 1.0, 2.0, 0.8])
    lo = np.zeros(d)
    hi = np.array([1.0, 2.5, 3.0, 2.0])
    mu = np.array([0.5 * sig[0], hi[1] - 0.5 * sig[1], 0.5 * sig[2], hi[3] - 0.5 * sig[3]])    # the mode 0.5 sigma from a face
    bounds = np.stack([lo, hi], axis=1)
    ll = lambda X: -0.5 * np.sum(((np.atleast_2d(X) - mu) / sig) ** 2, axis=1)      # noqa: E731
    gr = lambda X: -(np.atleast_2d(X) - mu) / sig ** 2                              # noqa: E731
    Xt = np.random.default_rng(4).uniform(lo, hi, (400, d))
    r = run_hmc(hr.HmcReflectNumpyDevice(ll, gr), bounds, 12, nchains, Xt, ll(Xt), reflect=True)
    assert r.converged and r.nreflect > 0
    m, se = _chain_means(r, nchains, d)
    ref = truncnorm.mean((lo - mu) / sig, (hi - mu) / sig, loc=mu, scale=sig)
    print(f"truncated Gaussian: eps = {r.eps:.3f}, nleap = {r.nleap}, acceptance = {r.acceptance:.3f}, {len(r.X)} rows, "
          f"{r.nreflect} reflections; max |mean - truncnorm| / se = {np.max(np.abs(m - ref) / se):.2f}")
    assert np.all((r.X >= lo) & (r.X <= hi))
    assert 0.5 < r.acceptance, r.acceptance
    assert np.all(np.abs(m - ref) < 5 * se), (m, ref, se)
