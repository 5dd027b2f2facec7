"""Maximum and profiles of the surrogate without a GPU: the numpy stand-in of the device call
(tests/tools/maximize_numpy.py) under the host code of gpry_amd/maximize.py, on analytic targets and on the oracle, and
what tests/test_maximize_gpu.py relies on: maximize_gp finds the mean of a Gaussian and the constrained maximum on a
wall; profile_gp gives the marginal forms, and with a continuation pass the upper envelope of a two-branch target; the
statuses; fixed coordinates keep their bits; ill-formed arguments raise; the replay's float64 noise floor (against long
double) is below the EPS_M the GPU tolerance is made from, and its margins leave out few enough steps of the walk table;
the end-to-end results on the oracle do not depend on the starts at the 1e-9 level."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import maximize_numpy as mn  # noqa: E402

from gpry_amd.maximize import MAX_STATUS, maximize_gp, profile_gp  # noqa: E402

GTOL = 1e-6


def _gauss(d, rho=0.6, diagonal=False):
    """Mean, covariance, log-density and gradient of N(m, C): C_ij = s_i s_j rho^|i - j| (diagonal: rho = 0)."""
    m = 0.3 + 0.1 * np.arange(d) / max(d - 1, 1)
    s = 0.5 + 0.5 * np.arange(d) / max(d - 1, 1)
    R = np.eye(d) if diagonal else rho ** np.abs(np.subtract.outer(np.arange(d), np.arange(d)))
    C = R * np.outer(s, s)
    P = np.linalg.inv(C)
    ll = lambda X: -0.5 * np.einsum("ni,ij,nj->n", np.atleast_2d(X) - m, P, np.atleast_2d(X) - m)      # noqa: E731
    gr = lambda X: -(np.atleast_2d(X) - m) @ P                                                          # noqa: E731
    return m, C, P, ll, gr


def _gpr(ll, gr, bounds, seed, n=300, minus_inf_value=-np.inf, around=None):
    """A training set as a run leaves it: a third uniform on the box, the rest a broad sample around the mode (1.5 C),
    so that its weighted covariance, the H0 of maximize_gp, is an estimate of the posterior's."""
    bounds = np.asarray(bounds, dtype=float)
    rng = np.random.default_rng(seed)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (n, len(bounds)))
    if around is not None:
        m, C = around
        X[n // 3:] = np.clip(rng.multivariate_normal(m, 1.5 * C, n - n // 3), bounds[:, 0], bounds[:, 1])
    return mn.HostGpr(mn.MaxNumpyDevice(ll, gr), X, ll(X), bounds, minus_inf_value)


def _lambda_min(P, span):
    """The smallest eigenvalue of the Hessian of -ll in unit-cube coordinates."""
    return float(np.min(np.linalg.eigvalsh(P * np.outer(span, span))))


@pytest.mark.parametrize("d", [1, 2, 5, 16])
def test_maximize_gp_finds_the_mean_of_a_gaussian(d):
    m, C, P, ll, gr = _gauss(d)
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = _gpr(ll, gr, bounds, d, around=(m, C))
    r = maximize_gp(gpr, nstarts=24, gtol=GTOL)
    span = bounds[:, 1] - bounds[:, 0]
    lam = _lambda_min(P, span)
    conv = r.status == mn.CONVERGED_G
    dist = np.linalg.norm((r.X_all - m) / span, axis=1)
    print(f"d={d}: statuses {np.bincount(r.status, minlength=6)}, iterations {r.iters.mean():.1f}, max distance of the "
          f"CONVERGED_G starts {dist[conv].max():.3e}, bound gtol / lambda_min = {GTOL / lam:.3e}")
    assert conv.sum() >= 12 and set(r.status) <= {mn.CONVERGED_G, mn.STALLED}
    assert np.all(dist[conv] <= GTOL / lam)
    assert np.linalg.norm((r.x - m) / span) <= GTOL / lam and r.y == np.max(r.y_all) and r.n_distinct == 1
    assert gpr.n_eval == r.ncalls.sum() and np.all(r.ngrad == r.iters + 1)
    assert np.all(np.max(np.abs(r.G_all[conv]), axis=1) <= GTOL)


@pytest.mark.parametrize("d", [1, 2, 5, 16])
def test_a_box_that_cuts_the_peak_off_gives_the_maximum_on_the_wall(d):
    """A diagonal covariance: the constrained maximiser is the mean clamped to the box, coordinate by coordinate."""
    m, C, P, ll, gr = _gauss(d, diagonal=True)
    bounds = np.array([[-4.0, 4.0]] * d)
    bounds[0] = [-4.0, 0.1]                      # the wall x_0 = 0.1 cuts the peak (m_0 = 0.3) off
    if d > 2:
        bounds[d - 1] = [0.6, 4.0]               # and so does x_{d-1} = 0.6 (m_{d-1} = 0.4)
    gpr = _gpr(ll, gr, bounds, 10 + d, around=(m, C))
    r = maximize_gp(gpr, nstarts=24, gtol=GTOL)
    xs = np.clip(m, bounds[:, 0], bounds[:, 1])
    span = bounds[:, 1] - bounds[:, 0]
    lam = _lambda_min(P, span)
    conv = r.status == mn.CONVERGED_G
    dist = np.linalg.norm((r.X_all - xs) / span, axis=1)
    print(f"d={d}: statuses {np.bincount(r.status, minlength=6)}, max distance {dist[conv].max():.3e}, bound {GTOL / lam:.3e}")
    assert conv.sum() >= 12
    assert np.all(dist[conv] <= GTOL / lam)
    assert np.all(r.X_all[conv][:, 0] == 0.1) and np.all(r.G_all[conv][:, 0] > 0)      # on the wall, pushed against it
    assert abs(r.y - ll(xs)[0]) <= GTOL ** 2 / (2 * lam)
    # with a full covariance the maximum still lies on the wall, and the gradient along it vanishes
    m, C, P, ll, gr = _gauss(d)
    r = maximize_gp(_gpr(ll, gr, bounds, 20 + d, around=(m, C)), nstarts=24, gtol=GTOL)
    conv = r.status == mn.CONVERGED_G
    assert conv.sum() >= 12 and np.all(r.X_all[conv][:, 0] == 0.1)
    assert np.all(np.abs(r.G_all[conv][:, 1:d - 1 if d > 2 else d]) <= GTOL)


@pytest.mark.parametrize("d", [2, 5, 16])
def test_profile_gp_gives_the_marginal_forms(d):
    m, C, P, ll, gr = _gauss(d)
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = _gpr(ll, gr, bounds, 30 + d, around=(m, C))
    span = bounds[:, 1] - bounds[:, 0]
    lam = _lambda_min(P, span)
    tol = GTOL ** 2 / (2 * lam)
    i = d // 2
    grid = np.linspace(-1.0, 1.5, 7)
    p = profile_gp(gpr, i, grid, nstarts=8, gtol=GTOL)
    exact = -0.5 * (grid - m[i]) ** 2 / C[i, i]
    conv = p.status == mn.CONVERGED_G
    print(f"d={d}: 1-D profile statuses {p.status}, max error {np.max(np.abs(p.y - exact)):.3e}, bound {tol:.3e}")
    assert conv.sum() >= 4 and p.grid.shape == (7, 1) and p.X.shape == (7, d)
    assert np.all(np.abs(p.y - exact)[conv] <= tol)
    np.testing.assert_array_equal(p.X[:, i], grid)
    assert gpr.n_eval == p.ncalls
    ij = (0, d - 1)
    g2 = np.array([[a, b] for a in (-0.5, 0.4, 1.0) for b in (-0.2, 0.5, 1.2)])
    p2 = profile_gp(gpr, ij, g2, nstarts=8, gtol=GTOL)
    S2 = C[np.ix_(ij, ij)]
    dl = g2 - m[list(ij)]
    exact2 = -0.5 * np.einsum("ni,ij,nj->n", dl, np.linalg.inv(S2), dl)
    conv = p2.status == mn.CONVERGED_G
    print(f"d={d}: 2-D profile statuses {p2.status}, max error {np.max(np.abs(p2.y - exact2)):.3e}")
    if d > 2:
        assert conv.sum() >= 5
        assert np.all(np.abs(p2.y - exact2)[conv] <= tol)
    else:                                        # (d = 2: both coordinates fixed, nothing to maximise)
        np.testing.assert_allclose(p2.y, exact2, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(p2.X[:, list(ij)], g2)


def _two_branches():
    """A mixture of two ridges along x_0, at x_1 = -1 (peak at x_0 = -1) and at x_1 = +1 (peak at x_0 = +1, higher by
    0.5): at a fixed x_0 the lower ridge stays a local maximum in x_1 while it is less than about 8 below the other."""
    s0, s1 = 1.0, 0.5

    def parts(X):
        X = np.atleast_2d(X)
        a = -0.5 * ((X[:, 0] + 1) ** 2 / s0 ** 2 + (X[:, 1] + 1) ** 2 / s1 ** 2)
        b = 0.5 - 0.5 * ((X[:, 0] - 1) ** 2 / s0 ** 2 + (X[:, 1] - 1) ** 2 / s1 ** 2)
        return X, a, b

    def ll(X):
        _, a, b = parts(X)
        return np.logaddexp(a, b)

    def gr(X):
        X, a, b = parts(X)
        wa = np.exp(a - np.logaddexp(a, b))[:, None]
        ga = -np.stack([(X[:, 0] + 1) / s0 ** 2, (X[:, 1] + 1) / s1 ** 2], axis=1)
        gb = -np.stack([(X[:, 0] - 1) / s0 ** 2, (X[:, 1] - 1) / s1 ** 2], axis=1)
        return wa * ga + (1 - wa) * gb
    return ll, gr


def test_continuation_returns_the_upper_envelope_of_a_two_branch_target():
    from scipy.optimize import minimize_scalar
    ll, gr = _two_branches()
    bounds = np.array([[-4.0, 4.0], [-3.0, 3.0]])
    # training points around the higher peak only: every independent ascent starts on the ridge x_1 = +1
    X = np.array([1.0, 1.0]) + 0.2 * np.random.default_rng(0).normal(size=(60, 2))
    gpr = mn.HostGpr(mn.MaxNumpyDevice(ll, gr), X, ll(X), bounds)
    # (in grid order; x_0 = -1 is the one row where the lower ridge still holds the ascents from x_1 = +1)
    grid = np.array([-3.5, -3.0, -1.0, 0.5, 1.0])
    env = np.array([max(-minimize_scalar(lambda t: -ll([[g, t]])[0], bounds=b, method="bounded",
                                         options=dict(xatol=1e-10)).fun for b in ((-3, 0), (0, 3))) for g in grid])
    p0 = profile_gp(gpr, 0, grid, nstarts=8, continuation=0)
    p1 = profile_gp(gpr, 0, grid, nstarts=8, continuation=1)
    print("envelope        ", np.round(env, 4))
    print("continuation = 0", np.round(p0.y, 4), "branch x_1", np.round(p0.X[:, 1], 2))
    print("continuation = 1", np.round(p1.y, 4), "branch x_1", np.round(p1.X[:, 1], 2))
    assert np.max(np.abs(p1.y - env)) < 1e-8
    assert np.max(env - p0.y) > 0.5, "the independent maximisations did not miss the envelope"
    assert np.all(p1.y >= p0.y) and p1.ncalls > p0.ncalls
    assert (p1.X[:, 1] < 0).any() and (p1.X[:, 1] > 0).any()


def _gated_plateau():
    """A Gaussian with a -inf half-space x_0 > 1 (the gate) and clipped at -0.5 (the plateau around the mode)."""
    m, C, P, ll0, gr = _gauss(2)

    def ll(X):
        X = np.atleast_2d(X)
        return np.where(X[:, 0] > 1.0, -np.inf, np.minimum(ll0(X), -0.5))
    return m, ll0, ll, gr


def test_statuses_on_a_gated_and_clipped_target():
    m, ll0, ll, gr = _gated_plateau()
    lo, hi = np.array([-4.0, -4.0]), np.array([4.0, 4.0])
    dev = mn.MaxNumpyDevice(ll, gr)
    X0 = np.array([[2.0, 0.0], [0.35, 0.3], [-2.0, -2.0], [0.9, -3.0], [-3.0, 3.0]])
    H0 = 30.0 * np.eye(2) / 64.0                 # long first steps: trial points cross the gate
    out = dev.maximize_mean(lo, hi, X0, np.full(5, np.nan), np.zeros(2, bool), H0, 50, 12, GTOL, 0.0, -np.inf, hooks=True)
    print("statuses", [MAX_STATUS[s] for s in out["status"]], "iterations", out["iters"], "gated trials", dev.gated_trials)
    assert out["status"][0] == mn.BAD_START and out["iters"][0] == 0 and out["ngrad"][0] == 0
    np.testing.assert_array_equal(out["X"][0], X0[0])
    assert np.isneginf(out["y"][0]) and np.all(np.isnan(out["G"][0]))
    assert out["status"][1] == mn.STALLED and out["iters"][1] == 0       # a start on the plateau: no trial improves y
    np.testing.assert_array_equal(out["X"][1], X0[1])
    assert np.all(out["status"][2:] == mn.STALLED)                        # the others climb until they reach the plateau
    assert np.all(out["y"][1:] == -0.5) and np.all(out["iters"][2:] > 0)
    assert dev.gated_trials > 0
    U = out["U_tr"][1:][~np.isnan(out["y_tr"][1:])]          # (every traced iterate but the gated start itself)
    assert np.all(lo[0] + U[:, 0] * (hi[0] - lo[0]) <= 1.0 + 1e-12) and np.all(out["X"][1:, 0] <= 1.0)
    assert np.all(np.isfinite(out["y_tr"][1:][~np.isnan(out["y_tr"][1:])]))
    # a start below minus_inf_value is a bad start too, and a given y0 is not evaluated again
    out = dev.maximize_mean(lo, hi, X0[2:4], np.array([-1000.0, np.nan]), np.zeros(2, bool), H0, 3, 12, GTOL, 0.0, -500.0)
    assert out["status"][0] == mn.BAD_START and out["ncalls"][0] == 0 and out["status"][1] != mn.BAD_START


def test_degenerate_masks_and_fixed_coordinates():
    m, C, P, ll, gr = _gauss(5)
    bounds = np.array([[-4.0, 4.0]] * 5)
    gpr = _gpr(ll, gr, bounds, 3, around=(m, C))
    r = maximize_gp(gpr, nstarts=8, fixed=np.ones(5, bool))
    np.testing.assert_array_equal(r.X_all, mn._Core(bounds[:, 0], bounds[:, 1], r.X_all, np.ones(5, bool), np.eye(5), 1, 0, 0,
                                                    -np.inf, None, np.float64).x)
    order = np.argsort(-gpr.y_train, kind="stable")[:8]
    np.testing.assert_array_equal(r.X_all, gpr.X_train[order])
    np.testing.assert_array_equal(r.y_all, gpr.y_train[order])
    assert np.all(r.iters == 0) and np.all(r.status == mn.CONVERGED_G) and np.all(r.ncalls == 1)
    for fixed in ([2], (0, 4), np.array([True, True, False, True, True])):
        r = maximize_gp(gpr, nstarts=8, fixed=fixed)
        mask = np.zeros(5, bool)
        mask[np.asarray(fixed)] = True
        np.testing.assert_array_equal(r.X_all[:, mask], gpr.X_train[order][:, mask])
        assert np.all(r.iters > 0) and np.all(np.any(r.X_all[:, ~mask] != gpr.X_train[order][:, ~mask], axis=1))
        # the conditional maximum of the free coordinates given the fixed ones
        A, B = P[np.ix_(~mask, ~mask)], P[np.ix_(~mask, mask)]
        xs = m[~mask] - np.linalg.solve(A, B @ (r.X_all[:, mask] - m[mask]).T).T
        assert np.max(np.abs(r.X_all[:, ~mask] - xs)) < 1e-5


def test_ill_formed_arguments_raise():
    m, C, P, ll, gr = _gauss(3)
    bounds = np.array([[-4.0, 4.0]] * 3)
    gpr = _gpr(ll, gr, bounds, 4, around=(m, C))
    with pytest.raises(TypeError):
        maximize_gp(gpr, bogus=1)
    with pytest.raises(TypeError):
        profile_gp(gpr, 0, [0.0], bogus=1)
    for kw in (dict(nstarts=0), dict(nstarts=2.5), dict(starts=np.zeros((2, 4))), dict(starts=[[9.0, 0.0, 0.0]]),
               dict(fixed=[3]), dict(fixed=[0, 0]), dict(fixed=[0.5]), dict(fixed=np.ones(2, bool)), dict(covmat=np.eye(2)),
               dict(covmat=-np.eye(3)), dict(max_iter=-1), dict(max_halvings=-1), dict(gtol=-1.0), dict(gtol=np.nan),
               dict(ftol=np.inf), dict(bounds=[[0.0, 0.0]] * 3)):
        with pytest.raises(ValueError):
            maximize_gp(gpr, **kw)
    for args, kw in (((3, [0.0]), {}), (((0, 0), [[0.0, 0.0]]), {}), ((0, [5.0]), {}), ((0, [[0.0, 1.0]]), {}),
                     (((0, 1), [0.0, 1.0, 2.0]), {}), ((0, []), {}), ((0, [0.0]), dict(nstarts=0)),
                     ((0, [0.0]), dict(continuation=-1)), ((0.5, [0.0]), {}), ((0, [np.nan]), {})):
        with pytest.raises(ValueError):
            profile_gp(gpr, *args, **kw)
    dev = gpr.device
    ok = (bounds[:, 0], bounds[:, 1], gpr.X_train[:2], np.full(2, np.nan), np.zeros(3, bool), np.eye(3), 5, 12, 1e-6, 0.0, -np.inf)
    dev.maximize_mean(*ok)
    for pos, bad in ((4, np.zeros(2, bool)), (5, np.eye(2)), (6, -1), (7, -1), (8, -1.0), (9, np.nan)):
        a = list(ok)
        a[pos] = bad
        with pytest.raises(ValueError):
            dev.maximize_mean(*a)
    # a caller's starts and covmat are used as given
    r = maximize_gp(gpr, starts=[[1.0, 1.0, 1.0]], covmat=C)
    assert len(r.y_all) == 1 and np.array_equal(dev.calls[-1]["X0"], [[1.0, 1.0, 1.0]])
    np.testing.assert_allclose(dev.calls[-1]["H0"], C / 64.0, rtol=1e-15)
    assert np.max(np.abs(r.x - m)) < 1e-5


# ---- the walk table ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    out = {}
    for name in mn.MAX_CASES:
        w = mn.Walk(name, gpr_device=OracleDevice())
        dev = mn.MaxNumpyDevice(w.loglike, w.grad_x)
        tr = dev.maximize_mean(*w.args(), hooks=True)
        out[name] = dict(w=w, tr=tr, rep=w.replay(tr), ld=w.replay(tr, dtype=np.longdouble), gated=dev.gated_trials)
    return out


def test_the_table_has_the_cases_the_walk_test_is_set(table):
    import sampler_walk as sw
    cases = mn._cases()
    models = [c["model"] for c in cases.values()]
    assert {m["d"] for m in models} >= {1, 3, 5, 9, 17, 32} and {m["N"] for m in models} >= {70, 1100, 2500}
    assert {m["kid"] for m in models} == {sw.RBF, sw.M12, sw.M32, sw.M52}
    assert {m.get("affine", True) for m in models} == {True, False} and any(m.get("svm") for m in models)
    nfixed = {(len(c.get("fixed", [])), c["model"]["d"]) for c in cases.values()}
    assert {n for n, _ in nfixed} >= {0, 1, 2} and any(n == d - 1 and n > 0 for n, d in nfixed)
    assert mn.MAX_ITER <= 6 and mn.REPLAY_TOL == 100 * mn.EPS_M
    assert (mn.LEFT_OUT_CASE, mn.LEFT_OUT_TABLE, mn.MARGIN) == (0.25, 0.05, 1e-9)
    # the wall case shrinks the free set and resets H; walls and corners start there; the gated case meets the gates
    e = table["wall cuts the peak"]
    assert np.sum(e["tr"]["reset_tr"] > 0) > 0 and np.all(e["tr"]["X"][e["tr"]["status"] == mn.CONVERGED_G][:, 0] == e["w"].hi[0])
    w = table["starts on walls and corners"]["w"]
    on = np.sum((w.X0 == w.lo) | (w.X0 == w.hi), axis=1)
    assert np.all(on >= 1) and np.any(on == 3)
    assert table["gated"]["gated"] > 0 and np.sum(table["gated"]["tr"]["nhalv_tr"] > 0) > 0
    for name, e in table.items():
        assert np.all(e["tr"]["iters"] <= mn.MAX_ITER) and np.sum(e["tr"]["iters"]) > 2 * mn.N_STARTS, name


def test_replay_follows_the_stand_in_and_noise_floor_and_left_out_shares(table):
    eps_m, left_all, ran_all = 0.0, 0, 0
    for name, e in table.items():
        tr, rep, ld = e["tr"], e["rep"], e["ld"]
        left, ran = mn.left_out(rep)
        left_all, ran_all = left_all + left, ran_all + ran
        keep = rep["ran"] & rep["keep"][:, :-1]
        step = keep & (tr["nhalv_tr"] >= 0)
        # the replay of the stand-in's own trace is the stand-in, bit for bit
        np.testing.assert_array_equal(rep["U_next"][step], tr["U_tr"][:, 1:][step], err_msg=name)
        np.testing.assert_array_equal(rep["nhalv"][keep], tr["nhalv_tr"][keep], err_msg=name)
        np.testing.assert_array_equal(rep["reset"][keep], tr["reset_tr"][keep], err_msg=name)
        np.testing.assert_array_equal(rep["end_iters"], tr["iters"], err_msg=name)
        np.testing.assert_array_equal(rep["end_status"], tr["status"], err_msg=name)
        both = step & ld["keep"][:, :-1]
        np.testing.assert_array_equal(rep["nhalv"][both], ld["nhalv"][both], err_msg=name)
        e_case = float(np.max(np.abs(rep["U_next"] - ld["U_next"])[both], initial=0.0))
        eps_m = max(eps_m, e_case)
        print(f"{name}: {left} of {ran} steps left out; statuses {np.bincount(tr['status'], minlength=6)}; "
              f"|U_f64 - U_longdouble| <= {e_case:.3g}")
        assert left <= mn.LEFT_OUT_CASE * ran, (name, left, ran)
    print(f"eps_m = {eps_m:.3g} (EPS_M = {mn.EPS_M:g}); {left_all} of {ran_all} steps left out")
    assert left_all <= mn.LEFT_OUT_TABLE * ran_all
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:      # (where long double is wider than double)
        assert 0.0 < eps_m <= mn.EPS_M, eps_m


# ---- end to end on the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mn.E2E_MODELS))
def test_the_oracle_side_results_do_not_depend_on_the_starts_at_the_1e_minus_9_level(name):
    m, gpr = mn.e2e_oracle(name)
    a = mn.e2e_results(gpr, m.d)
    m2, gpr2 = mn.e2e_oracle(name, perturb=1e-9)
    assert np.max(np.abs(gpr2.X_train - gpr.X_train)) > 1e-10
    b = mn.e2e_results(gpr2, m.d)
    tol = 2 * m.tol()
    print(f"{name}: best y {a[0].y:.6g} / {b[0].y:.6g}; max profile difference "
          f"{max(np.max(np.abs(a[1].y - b[1].y)), np.max(np.abs(a[2].y - b[2].y))):.3e}; tolerance {tol:.3e}")
    assert abs(a[0].y - b[0].y) <= tol
    assert np.max(np.abs(a[1].y - b[1].y)) <= tol and np.max(np.abs(a[2].y - b[2].y)) <= tol
    assert np.all(np.isfinite(a[1].y)) and np.all(np.isfinite(a[2].y))
    assert gpr.n_eval == a[0].ncalls.sum() + a[1].ncalls + a[2].ncalls
