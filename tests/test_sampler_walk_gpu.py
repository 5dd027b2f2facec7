"""The device samplers' walks, step by step, against host references that the device did not compute
(tests/tools/sampler_walk.py; likelihood: the float64 numpy oracle).

A. ns_chain_kernel: ``ns_generation(..., num_repeats=r)`` for r = 0 .. 8 with one seed and generation is the state of the
   same walk after each step; every state, evaluation count and y is compared with the traced numpy walk, at all 16
   (DP, kernel id) instantiations, with the x-affine on and off, the clip, the gates, narrow / wide W, a plateau, starts on
   faces, chains whose every try is gated, and the clustered / volumes variants.
B. mcmc_chain_kernel: the Metropolis rule of test_mcmc_gpu.py at the same instantiations, with thin > 1, y0 given, a
   finite minus_inf_value, a gated model, and the oracle as a second referee of every proposal's y.
C. ns_eval = one-point predict, bit for bit, and = the oracle within the suite's tolerance, at the edges of the slice
   layout (N = 1 .. 9217), through ns_prior and through mcmc_chains (starts on training rows and on the box's corners).

Wall time of this file on an MI355X: 26 s alone; the `-m gpu` suite took 267 s with it in the same session, 241 s without
(profiles/sampler_walk.md)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _proposal, _pushed
from test_nested_gpu import _one_point

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_philox  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

R, K = sw.R_STEPS, sw.N_CHAINS


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sw.NESTED_CASES))
def test_nested_chain_follows_the_reference_walk_step_by_step(name):
    g = sw.Generation(name)
    gpr = _pushed(g.gpr)
    dev = gpr.device
    tr = g.trace()
    span = g.hi - g.lo
    tol_y = g.model.tol()
    worst_u = worst_y = 0.0
    for r in range(R + 1):
        X, y, n, _ = g.device_call(dev, r)
        keep = tr.keep(r)
        where = f"{name}, step {r}: {int(np.sum(~keep))} of {K} chains left out"
        # the claim of nested.hip: y is the one-point predict of the returned point, bit for bit (every chain)
        moved = np.any(X != g.Xs[tr.start], axis=1) if r else np.zeros(K, bool)
        np.testing.assert_array_equal(y[moved], _one_point(gpr, X[moved]), err_msg=where)
        np.testing.assert_array_equal(y[~moved], g.ys[tr.start][~moved], err_msg=where)
        assert np.all((X >= g.lo) & (X <= g.hi)), where
        U = (X - g.lo) / span
        du = np.max(np.abs(U[keep] - tr.U[r][keep]), initial=0.0)
        worst_u = max(worst_u, du)
        assert du <= sw.POS_TOL, (where, du, np.flatnonzero(keep)[np.argmax(np.max(np.abs(U[keep] - tr.U[r][keep]), axis=1))])
        np.testing.assert_array_equal(n[keep], tr.ncalls[r][keep], err_msg=where)
        dy = np.max(np.abs(y[keep] - tr.y[r][keep]), initial=0.0)
        worst_y = max(worst_y, dy)
        assert dy <= tol_y, (where, dy)
        if r == 0:
            np.testing.assert_array_equal(X, g.Xs[tr.start], err_msg=where)
            np.testing.assert_array_equal(n, 0)
    left = int(np.sum(~tr.keep(R)))
    assert left <= sw.LEFT_OUT_CASE * K, f"{name}: {left} of {K} chains left out by step {R}"
    if g.variant == "narrow":
        capped = tr.stepout == ns_philox.STEP_OUT_MAX
        assert np.sum(capped & tr.keep(R)) > 0, "no compared chain reached the step-out cap"
    if g.variant in ("plateau", "gated"):
        np.testing.assert_array_equal(X, g.Xs[tr.start])
        np.testing.assert_array_equal(y, g.ys[tr.start])
        np.testing.assert_array_equal(n, tr.ncalls[R])
    # a second context runs the R-step call to the same bits
    gpr2 = _pushed(g.model.gpr())
    assert gpr2.device is not dev
    X2, y2, n2, _ = g.device_call(gpr2.device, R)
    np.testing.assert_array_equal(X2, X)
    np.testing.assert_array_equal(y2, y)
    np.testing.assert_array_equal(n2, n)
    print(f"{name}: compared {K - left} of {K} chains over {R} steps ({left} left out); max |du| = {worst_u:.2e} "
          f"(tolerance {sw.POS_TOL:.1e}), max |dy| = {worst_y:.2e} (tolerance {tol_y:.1e}); "
          f"{int(np.sum(tr.ncalls[R]))} evaluations, all counts equal")


# ---- B ----------------------------------------------------------------------------------------------------------------
def _rule_case(model, i, scale=1.0, T=1.0):
    gpr = _pushed(model.gpr())
    ref = model.oracle(gpr)
    mean = model.mean_fn(ref, gpr)
    clip = float(ref.clip_hi())
    bounds = model.bounds
    n, steps = 16, 40
    thin = 1 if i % 3 == 0 else 3                       # (40 % 3 != 0: the last step is not recorded)
    rng = np.random.default_rng(100 + i)
    X0 = np.ascontiguousarray(gpr.X_train[rng.choice(len(gpr.X_train), n)])
    y_true = _one_point(gpr, X0)
    if i % 2:
        y0 = y_start = y_true - 0.25                    # a given y0 is what the rule starts from, whatever predict says
    else:
        y0, y_start = np.full(n, np.nan), y_true
    miv = float(np.median(y_true)) - 3.0 if i % 4 == 2 else gpr.minus_inf_value
    counts = sw.check_metropolis_rule(gpr.device, bounds[:, 0], bounds[:, 1], X0, y0, y_start,
                                      _proposal(gpr, bounds, scale), T, miv, 4321 + i, i, steps, thin,
                                      oracle_y=lambda X: np.minimum(mean(X), clip), oracle_tol=model.tol())
    if i % 4 == 2:
        assert counts["below_minus_inf_value"] > 0, "no proposal the rule would take lay below minus_inf_value"
    print(counts)
    return counts


@pytest.mark.parametrize("i", range(len(sw.PLAIN_ROWS)))
def test_metropolis_rule_at_every_instantiation(i):
    d, kid, N, affine = sw.PLAIN_ROWS[i]
    counts = _rule_case(sw.Model(d, kid, N, affine=affine), i, scale=(3.0 if i % 5 == 3 else 1.0), T=(1.5 if i % 2 else 1.0))
    assert counts["accepted"] > 0 or N == 17


def test_metropolis_rule_with_the_gates():
    counts = _rule_case(sw.Model(3, sw.M52, 300, svm=True, seed=9), 3, scale=2.0)
    assert counts["gated"] > 0, "no proposal met the gates"


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,kid,affine", sw.EVAL_CASES)
def test_sampler_evaluation_equals_one_point_predict_at_the_edges_of_the_slice_layout(N, d, kid, affine):
    model = sw.eval_model(N, d, kid, affine)
    gpr = _pushed(model.gpr())
    ref = model.oracle()
    tol = model.tol()
    lo, hi = model.bounds[:, 0], model.bounds[:, 1]
    X, y, _ = gpr.device.ns_prior(lo, hi, 31 + N, 48)
    np.testing.assert_array_equal(X, ns_philox.prior_points(lo, hi, 31 + N, 48))
    np.testing.assert_array_equal(y, _one_point(gpr, X))
    assert np.max(np.abs(y - ref.predict(X))) <= tol
    # starts on training rows, on corners of the box and inside; a proposal far wider than the box: nothing moves, the
    # only evaluation of a chain is its start's
    corners = np.array([lo, hi, np.where(np.arange(d) % 2, lo, hi)])
    X0 = np.ascontiguousarray(np.concatenate([model.X[:3], corners, X[:4]]))
    n = len(X0)
    out = gpr.device.mcmc_chains(lo, hi, X0, np.full(n, np.nan), 1e3 * np.eye(d), 1.0, -np.inf, 7, 0, 2, 1, proposals=True)
    np.testing.assert_array_equal(out["X_last"], X0)
    np.testing.assert_array_equal(out["ncalls"], 1)
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, X0))
    assert np.max(np.abs(out["y_last"] - ref.predict(X0))) <= tol
    # and every evaluated proposal of a short walk
    out = gpr.device.mcmc_chains(lo, hi, X0, np.full(n, np.nan), 0.05 / np.sqrt(d) * np.eye(d), 1.0, -np.inf, 8, 1, 6, 1,
                                 proposals=True)
    ev = ~np.isnan(out["y_prop"].ravel())
    assert ev.sum() >= 6
    Xp, yp = out["X_prop"].reshape(-1, d)[ev], out["y_prop"].ravel()[ev]
    np.testing.assert_array_equal(yp, _one_point(gpr, Xp))
    assert np.max(np.abs(yp - ref.predict(Xp))) <= tol
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, out["X_last"]))
