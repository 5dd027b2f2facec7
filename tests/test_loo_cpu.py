"""Cross-validation of the training set without a GPU: the closed forms of tests/tools/loo_numpy.py (leave-one-out,
leave-group-out, one-step-ahead from V = L^-1 and alpha_) against brute-force refits in transformed space, the prior at
N = 1, the identities that tie the one-step-ahead predictives to the log marginal likelihood, and ``gpr.loo`` /
``gpr.leave_out`` / ``mc.validate_gp`` on a numpy device built from them (units, ``groups="last"``, the refusals, the
finite training set of an SVM model, a group whose block of K^-1 is not positive definite)."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import loo_numpy as ln  # noqa: E402
import sampler_walk as sw  # noqa: E402
from oracle import gpry_oracle as orc  # noqa: E402


class NumpyDevice(ln.NumpyLoo, OracleDevice):
    """The oracle-backed device with the two cross-validation calls."""


# every N once; d, the kernel id and the affine map go round as in COV_CASES of test_joint_gpu.py; N = 1 has no y scale
# to fit (normalize_y off); the last case has a noise level per point
CASES = [(N, (2, 9, 17, 32)[i % 4], (sw.RBF, sw.M32, sw.M52)[i % 3], i % 2 == 0, False) for i, N in enumerate((1, 17, 130, 400))]
CASES.append((130, 4, sw.RBF, True, True))
BRUTE_MAX = 40          # points refitted per case (all of them up to this many; spread over the set above)


def _case(N, d, kid, affine, per_point):
    noise = np.random.default_rng(N).uniform(5e-3, 5e-2, N) if per_point else 1e-2
    model = sw.Model(d, kid, N, affine=affine, normalize_y=N > 1, seed=N + d, noise_level=noise)
    ref = model.oracle()
    y_mean = float(ref.pre_y.inverse_transform(np.zeros(1))[0])
    y_std = float(ref.pre_y.inverse_transform_scale(np.ones(1))[0])
    K = orc.kernel_matrix(ref.X_train_, ref.theta, ref.kernel_id)
    K[np.diag_indices_from(K)] += ref.alpha
    return model, ref, K, y_mean, y_std


def _subset(N):
    return np.arange(N) if N <= BRUTE_MAX else np.unique(np.linspace(0, N - 1, BRUTE_MAX).astype(int))


def _groups(N, seed):
    rng = np.random.default_rng(seed)
    sizes = [s for s in (1, 15, 16, 17, 48, 64) if s <= N]
    groups = [rng.choice(N, s, replace=False) for s in sizes]
    if N > 2:
        groups.append(np.array([N - 1, 0, N // 2]))           # unsorted, and overlapping the others
    return groups


@pytest.mark.parametrize("N,d,kid,affine,per_point", CASES)
def test_closed_forms_against_brute_force_refits(N, d, kid, affine, per_point):
    """Bounds: the project's specification: the mean within MEAN_TOL max(1, max|y|), variances and
    group covariances within 1e-6 C y_std^2."""
    model, ref, K, y_mean, y_std = _case(N, d, kid, affine, per_point)
    unit = float(np.exp(model.theta[0])) * y_std ** 2
    res = ln.loo(ref.V_, ref.alpha_, ref.y_train_, ref.alpha, y_mean, y_std)
    sub = _subset(N)
    bm, bv = np.empty(len(sub)), np.empty(len(sub))
    sm, sv = np.empty(len(sub)), np.empty(len(sub))
    for k, i in enumerate(sub):
        m, c = ln.brute_leave_out(K, ref.y_train_, [i], y_mean, y_std)
        bm[k], bv[k] = m[0], c[0, 0]
        m, c = ln.brute_leave_out(K[:i + 1, :i + 1], ref.y_train_[:i + 1], [i], y_mean, y_std)
        sm[k], sv[k] = m[0], c[0, 0]
    e = dict(mean=np.max(np.abs(res["mean"][sub] - bm)), var_y=np.max(np.abs(res["var_y"][sub] - bv)),
             var_f=np.max(np.abs(res["var_f"][sub] - np.maximum(bv - ref.alpha[sub] * y_std ** 2, 0.0))),
             seq_mean=np.max(np.abs(res["seq_mean"][sub] - sm)), seq_var_y=np.max(np.abs(res["seq_var_y"][sub] - sv)))
    print(f"N={N} d={d} kid={kid} affine={affine} per-point noise={per_point}: cond K = {np.linalg.cond(K):.2e}; "
          f"mean {e['mean']:.2e}, seq_mean {e['seq_mean']:.2e} (bound {model.tol():.2e}); var_y {e['var_y'] / unit:.2e}, "
          f"var_f {e['var_f'] / unit:.2e}, seq_var_y {e['seq_var_y'] / unit:.2e} C y_std^2 (bound 1e-6)")
    assert e["mean"] <= model.tol() and e["seq_mean"] <= model.tol()
    assert max(e["var_y"], e["var_f"], e["seq_var_y"]) <= 1e-6 * unit
    groups = _groups(N, seed=N)
    out = ln.leave_out(ref.V_, ref.alpha_, ref.y_train_, groups, y_mean, y_std)
    y = ref.y_train_ * y_std + y_mean
    for k, g in enumerate(groups):
        m, c = ln.brute_leave_out(K, ref.y_train_, g, y_mean, y_std)
        em, ec = np.max(np.abs(out["mean"][k] - m)), np.max(np.abs(out["cov"][k] - c))
        r = y[g] - m
        chi2 = float(r.dot(np.linalg.solve(c, r)))
        lp = -0.5 * chi2 - 0.5 * np.linalg.slogdet(2 * np.pi * c)[1]
        print(f"  group of {len(g)}: mean {em:.2e} (bound {model.tol():.2e}), cov {ec / unit:.2e} C y_std^2 (bound 1e-6), "
              f"chi2 {out['chi2'][k]:.6g} / brute {chi2:.6g}, logpdf {out['logpdf'][k]:.6g} / brute {lp:.6g}")
        assert out["info"][k] == 0 and out["dof"][k] == len(g)
        assert em <= model.tol() and ec <= 1e-6 * unit
        # chi^2 and the log density of the brute-force predictive: the residual's error over its sigma, squared terms
        assert abs(out["chi2"][k] - chi2) <= 1e-6 * max(1.0, chi2)
        assert abs(out["logpdf"][k] - lp) <= 1e-6 * max(1.0, abs(lp))


def test_a_single_training_point_gives_the_prior():
    model, ref, K, _, _ = _case(1, 2, sw.RBF, True, False)
    C, noise = float(np.exp(model.theta[0])), float(ref.alpha[0])
    res = ln.loo(ref.V_, ref.alpha_, ref.y_train_, ref.alpha, y_mean=2.5, y_std=3.0)
    for key in ("mean", "seq_mean"):
        np.testing.assert_allclose(res[key], [2.5], rtol=0, atol=1e-14 * abs(ref.y_train_[0] * 3.0))
    for key in ("var_y", "seq_var_y"):
        np.testing.assert_allclose(res[key], [(C + noise) * 9.0], rtol=1e-14)
    np.testing.assert_allclose(res["var_f"], [C * 9.0], rtol=1e-14)
    out = ln.leave_out(ref.V_, ref.alpha_, ref.y_train_, [[0]], 2.5, 3.0)
    np.testing.assert_allclose(out["mean"][0], [2.5], rtol=0, atol=1e-14 * abs(ref.y_train_[0] * 3.0))
    np.testing.assert_allclose(out["cov"][0], [[(C + noise) * 9.0]], rtol=1e-14)


@pytest.mark.parametrize("N,d,kid,affine,per_point", CASES)
def test_one_step_ahead_sums_to_the_log_marginal_likelihood(N, d, kid, affine, per_point):
    """sum_k log N(y_k; seq_mean_k, seq_var_k) = LML at the same theta, within the tolerance tests/test_oracle_golden.py
    holds the oracle's LML to (1e-12 relative); sum_k z_k^2 = y_^T K^-1 y_ = y_^T alpha_, within the rounding of the two
    length-N sums and of the solve behind alpha_ (u cond(K) relative to |y_| |alpha_|: Higham 10.1)."""
    model, ref, K, _, _ = _case(N, d, kid, affine, per_point)
    res = ln.loo(ref.V_, ref.alpha_, ref.y_train_, ref.alpha)
    lml = float(orc.log_marginal_likelihood(ref.X_train_, ref.y_train_, ref.alpha, ref.theta, ref.kernel_id))
    total = float(np.sum(ln.log_density(ref.y_train_, res["seq_mean"], res["seq_var_y"])))
    z = (ref.y_train_ - res["seq_mean"]) / np.sqrt(res["seq_var_y"])
    quad, ya = float(z.dot(z)), float(ref.y_train_.dot(ref.alpha_))
    np.testing.assert_allclose(z, res["w"], rtol=0, atol=1e-9 * max(1.0, np.max(np.abs(res["w"]))))
    bound = 2.0 ** -53 * (4 * (N + 2) * (quad + np.abs(ref.y_train_).dot(np.abs(ref.alpha_)))
                          + 8 * N * np.linalg.cond(K) * np.linalg.norm(ref.y_train_) * np.linalg.norm(ref.alpha_))
    print(f"N={N} d={d} kid={kid}: sum of log densities {total:.15g}, LML {lml:.15g}, difference {abs(total - lml):.2e} "
          f"(bound {1e-12 * abs(lml):.2e}); sum z^2 {quad:.15g}, y.alpha_ {ya:.15g}, difference {abs(quad - ya):.2e} "
          f"(bound {bound:.2e})")
    assert abs(total - lml) <= 1e-12 * abs(lml)
    assert abs(quad - ya) <= bound


def test_the_class_units_groups_last_and_refusals():
    from gpry_amd import mc
    from gpry_amd._lib import GpryHipError
    model = sw.Model(3, sw.M52, 45, seed=4)
    full = sw.Model(3, sw.M52, 45, seed=4)
    model.X, model.y = full.X[:40], full.y[:40]
    gpr = model.gpr(device=NumpyDevice())
    gpr._ensure_factor()
    gpr.append_to_data(full.X[40:], full.y[40:], fit_gpr=False, fit_classifier=False)      # frozen pre-processors: a border update
    assert gpr.n_border_updates == 1 and len(gpr.y_train) == 45 and gpr.n_last_appended_finite == 5
    y_mean, y_std = gpr._y_affine()
    V, a = gpr.device._factor[1], gpr.device._factor[2]
    want = ln.loo(V, a, gpr.y_train_, gpr.alpha, y_mean, y_std)
    n0 = gpr.n_eval
    res = gpr.loo()
    assert gpr.n_eval == n0                                 # nothing is evaluated: the training set is the data
    for key in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y"):
        assert res[key].shape == (45,)
        np.testing.assert_array_equal(res[key], want[key])
    # units: the transformed-space predictive mapped by the y pre-processor
    raw = ln.loo(V, a, gpr.y_train_, gpr.alpha)
    np.testing.assert_allclose(res["mean"], gpr.preprocessing_y.inverse_transform(raw["mean"]), rtol=1e-13)
    np.testing.assert_allclose(res["var_y"], gpr.preprocessing_y.inverse_transform_scale(np.sqrt(raw["var_y"])) ** 2, rtol=1e-13)
    assert np.all(res["var_f"] < res["var_y"]) and np.all(res["var_f"] >= 0)
    # groups="last": the five points of the border update, as one group
    last = gpr.leave_out("last")
    assert len(last["groups"]) == 1
    np.testing.assert_array_equal(last["groups"][0], np.arange(40, 45))
    explicit = gpr.leave_out([[40, 41, 42, 43, 44], [44, 40, 41, 43, 42]])
    np.testing.assert_array_equal(last["cov"][0], explicit["cov"][0])
    perm = [4, 0, 1, 3, 2]
    np.testing.assert_allclose(explicit["mean"][1], explicit["mean"][0][perm], rtol=1e-12)
    np.testing.assert_allclose(explicit["cov"][1], explicit["cov"][0][np.ix_(perm, perm)], rtol=1e-10)
    np.testing.assert_allclose(explicit["chi2"][1], explicit["chi2"][0], rtol=1e-10)
    assert last["dof"][0] == 5 and last["cov"][0].shape == (5, 5)
    r = gpr.y_train[40:] - last["mean"][0]
    np.testing.assert_allclose(last["chi2"][0], r.dot(np.linalg.solve(last["cov"][0], r)), rtol=1e-8)
    np.testing.assert_allclose(last["logpdf"][0], -0.5 * last["chi2"][0] - 0.5 * np.linalg.slogdet(2 * np.pi * last["cov"][0])[1],
                               rtol=1e-10)
    # the four refusals of the device, a wrong word, and a model without data
    for bad, word in (([[0, 1], []], "empty"), ([list(range(45)) + list(range(20))], "at most 64"), ([[0, 45]], "outside"),
                      ([[-1]], "outside"), ([[3, 7, 3]], "more than once")):
        with pytest.raises(GpryHipError, match=word):
            gpr.leave_out(bad)
    with pytest.raises(ValueError, match="last"):
        gpr.leave_out("first")
    from gpry_amd.gpr import GaussianProcessRegressor
    empty = GaussianProcessRegressor(kernel="RBF", bounds=model.bounds)
    for call in (empty.loo, lambda: empty.leave_out([[0]]), lambda: mc.validate_gp(empty)):
        with pytest.raises(ValueError, match="training data"):
            call()
    nothing = sw.Model(3, sw.M52, 30, seed=1).gpr(device=NumpyDevice())
    nothing.n_last_appended_finite = 0
    with pytest.raises(ValueError, match="no finite point"):
        nothing.leave_out("last")
    fresh = NumpyDevice()
    for call in (fresh.loo, lambda: fresh.leave_out([[0]])):
        with pytest.raises(GpryHipError, match="factor"):
            call()


def test_validate_gp_is_a_pure_report():
    from gpry_amd import mc
    model = sw.Model(2, sw.M52, 120, seed=3)
    model.y = model.y.copy()
    model.y[100] += 40.0                                    # one target that its neighbours contradict
    gpr = model.gpr(device=NumpyDevice())
    theta0 = gpr.kernel_.theta.copy()
    groups = [np.arange(60, 80), [101, 100, 99], [5]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep = mc.validate_gp(gpr, groups=groups)
        plain = mc.validate_gp(gpr)
    assert plain.groups is None and rep.n == 120 and "GPValidation" in repr(rep)
    np.testing.assert_array_equal(gpr.kernel_.theta, theta0)
    res = gpr.loo()
    for part, mk, vk in ((rep.loo, "mean", "var_y"), (rep.seq, "seq_mean", "seq_var_y")):
        z = (gpr.y_train - res[mk]) / np.sqrt(res[vk])
        np.testing.assert_array_equal(part["z"], z)
        assert part["rms"] == pytest.approx(np.sqrt(np.mean(z ** 2)), rel=1e-14)
        assert part["frac1"] == np.mean(np.abs(z) <= 1) and part["frac2"] == np.mean(np.abs(z) <= 2)
        np.testing.assert_array_equal(part["outliers"], np.flatnonzero(np.abs(z) > 3))
        assert part["mean_logpdf"] == pytest.approx(np.mean(ln.log_density(gpr.y_train, res[mk], res[vk])), rel=1e-13)
    assert 100 in rep.loo["outliers"] and 100 in rep.seq["outliers"]
    assert rep.GAUSS1 == pytest.approx(0.6827, abs=1e-4) and rep.GAUSS2 == pytest.approx(0.9545, abs=1e-4)
    g = rep.groups
    np.testing.assert_array_equal(g["dof"], [20, 3, 1])
    assert g["chi2"].shape == g["logpdf"].shape == (3,) and not g["info"].any()
    assert g["chi2"][1] > 9.0 * 3                          # the group that holds the contradicted point
    np.testing.assert_allclose(g["chi2"][2], rep.loo["z"][5] ** 2, rtol=1e-9)       # a group of one is leave-one-out
    for a, b in zip(g["indices"], groups):
        np.testing.assert_array_equal(a, b)


def test_indices_refer_to_the_finite_training_set_of_an_svm_model():
    model = sw.Model(3, sw.M52, 300, svm=True, seed=9)
    gpr = model.gpr(device=NumpyDevice())
    n = len(gpr.y_train)
    assert n < 300 and np.all(np.isfinite(gpr.y_train))
    ref = model.oracle(gpr)
    y_mean = float(ref.pre_y.inverse_transform(np.zeros(1))[0])
    y_std = float(ref.pre_y.inverse_transform_scale(np.ones(1))[0])
    want = ln.loo(ref.V_, ref.alpha_, ref.y_train_, ref.alpha, y_mean, y_std)
    res = gpr.loo()
    assert res["mean"].shape == (n,)
    unit = float(np.exp(model.theta[0])) * y_std ** 2
    np.testing.assert_allclose(res["mean"], want["mean"], rtol=0, atol=model.tol())
    np.testing.assert_allclose(res["var_y"], want["var_y"], rtol=0, atol=1e-6 * unit)
    out = gpr.leave_out([[n - 1, 0]])
    K = orc.kernel_matrix(ref.X_train_, ref.theta, ref.kernel_id)
    K[np.diag_indices_from(K)] += ref.alpha
    m, c = ln.brute_leave_out(K, ref.y_train_, [n - 1, 0], y_mean, y_std)
    np.testing.assert_allclose(out["mean"][0], m, rtol=0, atol=model.tol())
    np.testing.assert_allclose(out["cov"][0], c, rtol=0, atol=1e-6 * unit)
    with pytest.raises(Exception, match="outside"):
        gpr.leave_out([[n]])                                 # an index of the full set, beyond the finite one


def test_a_block_that_is_not_positive_definite_is_that_groups_alone():
    """On the device B = V_G^T V_G of a valid factor is positive definite by construction, so ``info`` != 0 is reached
    here, through the stand-in, with a factor whose column 5 was cleared."""
    model = sw.Model(2, sw.M52, 40, seed=2)
    gpr = model.gpr(device=NumpyDevice())
    gpr._ensure_factor()
    L, V, a = gpr.device._factor
    V = V.copy()
    V[:, 5] = 0.0
    gpr.device._factor = (L, V, a)
    out = gpr.leave_out([[1, 2, 3], [4, 5, 6], [5], [7, 8]])
    np.testing.assert_array_equal(out["info"] != 0, [False, True, True, False])
    for k in (1, 2):
        assert np.all(np.isnan(out["mean"][k])) and np.all(np.isnan(out["cov"][k]))
        assert np.isnan(out["chi2"][k]) and np.isnan(out["logpdf"][k])
    for k in (0, 3):
        assert np.all(np.isfinite(out["mean"][k])) and np.all(np.isfinite(out["cov"][k])) and np.isfinite(out["chi2"][k])
