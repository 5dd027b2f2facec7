"""Cross-validation of the training set on the device (gpry_amd/csrc/loo.hip, Device.loo / leave_out,
GaussianProcessRegressor.loo / leave_out, gpry_amd/mc.py: validate_gp): the device against the numpy closed forms of
tests/tools/loo_numpy.py evaluated on the factor fetched from the same context, within the forward bound of a length-N sum
taken in two orders; against brute-force refits at the project's specification; the bits (contexts, outputs asked for,
company, position and order of a group); groups of every padded size, overlapping, a partition; the factor grown by
gpry_append_rows; a Kriging-believer session around the calls; the log marginal likelihood; the refusals.

``info`` != 0 of a group is not reached here: B = V_G^T V_G of a valid factor is positive definite by construction and the
library offers no way to push a factor, so that branch is covered through the numpy stand-in in tests/test_loo_cpu.py."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import loo_numpy as ln  # noqa: E402
import sampler_walk as sw  # noqa: E402
from oracle import gpry_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_CACHE = {}
OUTPUTS = ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")


class Case:
    """A model on the device with its factor fetched once: V, alpha_, the transformed targets, the noise vector, the y map,
    the numpy closed form on that factor and the device's own ``loo``."""

    def __init__(self, d, kid, N, affine):
        self.model = sw.Model(d, kid, N, affine=affine, normalize_y=N > 1, seed=N + d)
        self.gpr = _pushed(self.model.gpr())
        self.dev = self.gpr.device
        _, self.V, self.a = self.dev.get_factor(want_L=False)
        self.y_, self.noise = self.gpr.y_train_, np.broadcast_to(self.gpr.alpha, (N,))
        self.y_mean, self.y_std = self.gpr._y_affine()
        self.unit = float(np.exp(self.model.theta[0])) * self.y_std ** 2
        self.ref = ln.loo(self.V, self.a, self.y_, self.noise, self.y_mean, self.y_std)
        self.out = self.dev.loo()

    def numpy_groups(self, groups):
        return ln.leave_out(self.V, self.a, self.y_, groups, self.y_mean, self.y_std)


def _case(N, i=0):
    """d, the kernel id and the affine map go round with i as in COV_CASES of test_joint_gpu.py."""
    key = (N, i)
    if key not in _CACHE:
        _CACHE[key] = Case((2, 9, 17, 32)[i % 4], (sw.RBF, sw.M32, sw.M52)[i % 3], N, i % 2 == 0)
    return _CACHE[key]


SIZES = (1, 17, 127, 128, 129, 600, 1100, 2500)


@pytest.mark.parametrize("i,N", list(enumerate(SIZES)))
def test_loo_against_the_closed_form_on_the_fetched_factor(i, N):
    """q_i and w_k are length-N sums taken in another order than numpy's: |dq_i| <= rho q_i and |dw_k| <= rho S_k with
    rho = 2 (N + 2) u and S_k = sum_i |V_ki y_i|.  Propagated to first order, with 4 u for the few roundings behind each
    output: var_y = y_std^2 / q by (rho + 4 u) var_y; var_f the same in units of y_std^2 / q; mean by
    y_std |alpha_i / q_i| (rho + 4 u) + 4 u (|y_i| y_std + |mean|); seq_mean by y_std (rho S_k + 4 u |w_k|) / V_kk + 4 u (|y_k|
    y_std + |seq_mean|); seq_var_y = y_std^2 / V_kk^2, no sum behind it, by 6 u seq_var_y."""
    c = _case(N, i)
    ref, out = c.ref, c.out
    rho, ys = 2 * (N + 2) * U, c.y_std
    S = np.abs(np.tril(c.V)).dot(np.abs(c.y_))
    bound = dict(var_y=(rho + 4 * U) * ref["var_y"], var_f=(rho + 4 * U) * ys ** 2 / ref["q"] + 4 * U * ref["var_f"],
                 mean=ys * np.abs(c.a / ref["q"]) * (rho + 4 * U) + 4 * U * (np.abs(c.y_) * ys + np.abs(ref["mean"])),
                 seq_mean=ys * (rho * S + 4 * U * np.abs(ref["w"])) / ref["vdiag"] + 4 * U * (np.abs(c.y_) * ys + np.abs(ref["seq_mean"])),
                 seq_var_y=6 * U * ref["seq_var_y"])
    ratio = {k: float(np.max(np.abs(out[k] - ref[k]) / bound[k])) for k in OUTPUTS}
    print(f"N={N} d={c.model.d} kid={c.model.kid} affine={c.model.affine}: |device - closed form| / bound: "
          + ", ".join(f"{k} {ratio[k]:.3f}" for k in OUTPUTS) + f"; device {out['device_ms']:.3f} ms")
    for k in OUTPUTS:
        assert out[k].shape == (N,) and ratio[k] <= 1.0, (k, ratio[k])
    assert np.all(out["var_f"] >= 0) and np.all(out["var_y"] > 0)


def test_a_single_training_point_gives_the_prior():
    c = _case(1, 0)
    dev = c.dev
    dev.set_affine(*c.gpr._affine_args()[:2], y_mean=2.5, y_std=3.0)
    try:
        out = dev.loo()
        grp = dev.leave_out([[0]])
    finally:
        dev.set_affine(*c.gpr._affine_args())
    C, noise = float(np.exp(c.model.theta[0])), float(c.noise[0])
    for k in ("mean", "seq_mean"):
        assert abs(out[k][0] - 2.5) <= 8 * U * abs(3.0 * c.y_[0])
    for k in ("var_y", "seq_var_y"):
        assert abs(out[k][0] - (C + noise) * 9.0) <= 8 * U * (C + noise) * 9.0
    assert abs(out["var_f"][0] - C * 9.0) <= 8 * U * (C + noise) * 9.0
    assert abs(grp["mean"][0][0] - 2.5) <= 8 * U * abs(3.0 * c.y_[0])
    assert abs(grp["cov"][0][0, 0] - (C + noise) * 9.0) <= 8 * U * (C + noise) * 9.0


def _group_set(N, seed):
    rng = np.random.default_rng(seed)
    groups = [rng.choice(N, s, replace=False) for s in (1, 15, 16, 17, 48, 64) if s <= N]
    if N > 2:
        groups.append(np.array([N - 1, 0, N // 2]))               # unsorted; overlaps the others
        groups.append(groups[-2][::-1].copy())
    return groups


@pytest.mark.parametrize("i,N", [(1, 17), (2, 130), (3, 400)])
def test_the_device_against_brute_force_refits(i, N):
    """The rows (and columns) of C k(X_, X_) + diag(noise) deleted and the rest solved, theta and the pre-processors
    frozen; bounds: the project's specification, the mean within MEAN_TOL max(1, max|y|), variances
    and group covariances within 1e-6 C y_std^2."""
    c = _case(N, i)
    g = c.gpr
    K = orc.kernel_matrix(g.X_train_, c.model.theta, c.model.kid)
    K[np.diag_indices_from(K)] += c.noise
    sub = np.arange(N) if N <= 40 else np.unique(np.linspace(0, N - 1, 40).astype(int))
    e = dict.fromkeys(OUTPUTS, 0.0)
    for k in sub:
        m, v = ln.brute_leave_out(K, c.y_, [k], c.y_mean, c.y_std)
        sm, sv = ln.brute_leave_out(K[:k + 1, :k + 1], c.y_[:k + 1], [k], c.y_mean, c.y_std)
        vf = max(v[0, 0] - c.noise[k] * c.y_std ** 2, 0.0)
        for name, val in (("mean", m[0]), ("var_y", v[0, 0]), ("var_f", vf), ("seq_mean", sm[0]), ("seq_var_y", sv[0, 0])):
            e[name] = max(e[name], abs(c.out[name][k] - val))
    tol = c.model.tol()
    print(f"N={N}: mean {e['mean']:.2e}, seq_mean {e['seq_mean']:.2e} (bound {tol:.2e}); var_y {e['var_y'] / c.unit:.2e}, "
          f"var_f {e['var_f'] / c.unit:.2e}, seq_var_y {e['seq_var_y'] / c.unit:.2e} C y_std^2 (bound 1e-6)")
    assert e["mean"] <= tol and e["seq_mean"] <= tol
    assert max(e["var_y"], e["var_f"], e["seq_var_y"]) <= 1e-6 * c.unit
    groups = _group_set(N, N)
    out = c.dev.leave_out(groups)
    for k, grp in enumerate(groups):
        m, cv = ln.brute_leave_out(K, c.y_, grp, c.y_mean, c.y_std)
        em, ec = float(np.max(np.abs(out["mean"][k] - m))), float(np.max(np.abs(out["cov"][k] - cv)))
        print(f"  group of {len(grp)}: mean {em:.2e} (bound {tol:.2e}), cov {ec / c.unit:.2e} C y_std^2 (bound 1e-6)")
        assert out["info"][k] == 0 and em <= tol and ec <= 1e-6 * c.unit


def _check_groups(c, groups, out, label):
    """Against the closed form on the fetched factor.  Mean and covariance at the specification; chi^2 and the log
    density, which have none, within the first-order bound of solving with a B whose entries are sums taken in another
    order: relative 8 n (N + 2 + 8 n) u cond(B) for chi^2 (the Gram's rho = 2 (N + 2) u entrywise against |V_G|^T |V_G|, whose
    norm is at most n |B|, and the n x n Cholesky solve's own 8 n u behind it), the same times chi^2 / 2 + n for the log density."""
    ref = c.numpy_groups(groups)
    tol, N = c.model.tol(), len(c.y_)
    worst = dict(mean=0.0, cov=0.0, chi2=0.0, logpdf=0.0)
    for k, g in enumerate(groups):
        n = len(g)
        VG = np.tril(c.V)[:, g]
        rel = 8 * n * (N + 2 + 8 * n) * U * np.linalg.cond(VG.T.dot(VG))
        assert out["info"][k] == 0 and out["dof"][k] == n and out["cov"][k].shape == (n, n)
        np.testing.assert_array_equal(out["cov"][k], out["cov"][k].T)
        worst["mean"] = max(worst["mean"], float(np.max(np.abs(out["mean"][k] - ref["mean"][k]))) / tol)
        worst["cov"] = max(worst["cov"], float(np.max(np.abs(out["cov"][k] - ref["cov"][k]))) / (1e-6 * c.unit))
        worst["chi2"] = max(worst["chi2"], abs(out["chi2"][k] - ref["chi2"][k]) / (rel * max(1.0, ref["chi2"][k])))
        worst["logpdf"] = max(worst["logpdf"], abs(out["logpdf"][k] - ref["logpdf"][k]) / (rel * (ref["chi2"][k] / 2 + n)))
    print(f"{label}: {len(groups)} groups, |device - closed form| / bound: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; device {out['device_ms']:.3f} ms")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("i,N", [(1, 17), (4, 129), (5, 600), (7, 2500)])
def test_groups_against_the_closed_form(i, N):
    """Sizes 1, 15, 16, 17, 48 and 64 (every padded size and both sides of a tile edge), overlapping, unsorted."""
    c = _case(N, i)
    groups = _group_set(N, 3 * N)
    _check_groups(c, groups, c.dev.leave_out(groups), f"N={N}")


def test_a_group_of_one_is_the_leave_one_out_entry():
    c = _case(600, 5)
    N = 600
    idx = np.array([0, 1, 63, 64, 255, 256, 257, 599])
    out = c.dev.leave_out([[k] for k in idx])
    rho = 2 * (N + 2) * U
    q = c.ref["q"][idx]
    b_var = 2 * (rho + 4 * U) * c.ref["var_y"][idx]
    b_mean = 2 * (c.y_std * np.abs(c.a[idx] / q) * (rho + 4 * U) + 4 * U * (np.abs(c.y_[idx]) * c.y_std + np.abs(c.ref["mean"][idx])))
    var = np.array([cv[0, 0] for cv in out["cov"]])
    mean = np.array([m[0] for m in out["mean"]])
    z2 = (c.gpr.y_train[idx] - c.out["mean"][idx]) ** 2 / c.out["var_y"][idx]
    print(f"group of one against loo: var {np.max(np.abs(var - c.out['var_y'][idx]) / b_var):.3f}, "
          f"mean {np.max(np.abs(mean - c.out['mean'][idx]) / b_mean):.3f} of the bound (two sums, each within rho)")
    assert np.all(np.abs(var - c.out["var_y"][idx]) <= b_var)
    assert np.all(np.abs(mean - c.out["mean"][idx]) <= b_mean)
    np.testing.assert_allclose(out["chi2"], z2, rtol=1e-9)


def test_a_partition_into_batches():
    """N = 600 as an initial design of 12 points and 147 batches of 4, every point in exactly one group."""
    c = _case(600, 5)
    groups = [np.arange(12)] + [np.arange(k, k + 4) for k in range(12, 600, 4)]
    assert sum(len(g) for g in groups) == 600 and len(groups) == 148
    out = c.dev.leave_out(groups)
    _check_groups(c, groups, out, "partition of 600")
    rep_groups = c.gpr.leave_out(groups)
    np.testing.assert_array_equal(rep_groups["chi2"], out["chi2"])
    from gpry_amd import mc
    rep = mc.validate_gp(c.gpr, groups=groups)
    np.testing.assert_array_equal(rep.groups["chi2"], out["chi2"])
    np.testing.assert_array_equal(rep.loo["z"], (c.gpr.y_train - c.out["mean"]) / np.sqrt(c.out["var_y"]))
    assert rep.n == 600 and rep.groups["dof"].sum() == 600


def test_the_bits_depend_on_the_model_and_the_group_alone():
    """N = 2500: forty row tiles of the pass, ten chunks of the Gram.  A second context; one output asked for; a group
    alone, among 300 others, at another place in the list, with its indices permuted."""
    c = _case(2500, 7)
    other = _pushed(c.model.gpr())
    assert other.device is not c.dev
    again = other.device.loo()
    for k in OUTPUTS:
        np.testing.assert_array_equal(again[k], c.out[k], err_msg=k)
        one = c.dev.loo(want=(k,))
        assert all(one[j] is None for j in OUTPUTS if j != k)
        np.testing.assert_array_equal(one[k], c.out[k], err_msg=k)
    rng = np.random.default_rng(11)
    crowd = [rng.choice(2500, int(s), replace=False) for s in rng.integers(1, 65, 300)]
    probes = [np.array([2499, 3, 1200, 700]), rng.choice(2500, 64, replace=False), rng.choice(2500, 17, replace=False),
              np.array([2400, 2300])]
    for p in probes:
        alone = c.dev.leave_out([p])
        for pos in (0, 150, 300):
            many = c.dev.leave_out(crowd[:pos] + [p] + crowd[pos:])
            for k in ("mean", "cov"):
                np.testing.assert_array_equal(many[k][pos], alone[k][0])
            for k in ("chi2", "logpdf", "info"):
                assert many[k][pos] == alone[k][0]
        far = other.device.leave_out([p])
        np.testing.assert_array_equal(far["cov"][0], alone["cov"][0])
        perm = rng.permutation(len(p))
        shuffled = c.dev.leave_out([p[perm]])
        np.testing.assert_array_equal(shuffled["mean"][0], alone["mean"][0][perm])
        np.testing.assert_array_equal(shuffled["cov"][0], alone["cov"][0][np.ix_(perm, perm)])
        assert shuffled["chi2"][0] == alone["chi2"][0] and shuffled["logpdf"][0] == alone["logpdf"][0]
    _check_groups(c, crowd, c.dev.leave_out(crowd), "300 groups at N=2500")


def test_after_append_rows_the_grown_factor_serves():
    """584 points factorised and 16 appended against the 600 factorised afresh, the same theta and y map on both sides:
    the specification's tolerances (the border update is another route to the same factor)."""
    from gpry_amd._lib import Device
    c = _case(600, 5)
    g = c.gpr
    kid, theta = g._device_theta()
    dev = Device(c.dev.device)
    try:
        dev.set_train(g.X_train_[:584], g.y_train_[:584], c.noise[:584])
        dev.set_theta(kid, theta)
        dev.set_affine(*g._affine_args())
        assert dev.factorize() == 0
        assert dev.append_rows(g.X_train_[584:], g.y_train_[584:], c.noise[584:]) == 0 and dev.N == 600
        out = dev.loo()
        groups = [np.arange(584, 600), np.array([599, 0, 300]), np.arange(560, 600)]
        grp, want = dev.leave_out(groups), c.dev.leave_out(groups)
    finally:
        dev.close()
    tol = c.model.tol()
    e_mean = max(float(np.max(np.abs(out[k] - c.out[k]))) for k in ("mean", "seq_mean"))
    e_var = max(float(np.max(np.abs(out[k] - c.out[k]))) for k in ("var_y", "var_f", "seq_var_y"))
    g_mean = max(float(np.max(np.abs(a - b))) for a, b in zip(grp["mean"], want["mean"]))
    g_cov = max(float(np.max(np.abs(a - b))) for a, b in zip(grp["cov"], want["cov"]))
    print(f"appended against fresh: means {e_mean:.2e}, group means {g_mean:.2e} (bound {tol:.2e}); variances "
          f"{e_var / c.unit:.2e}, group covariances {g_cov / c.unit:.2e} C y_std^2 (bound 1e-6)")
    assert e_mean <= tol and g_mean <= tol
    assert e_var <= 1e-6 * c.unit and g_cov <= 1e-6 * c.unit
    assert not grp["info"].any()


def test_a_kriging_believer_session_is_not_disturbed():
    """Candidates registered before the calls, and after them, give the Gram rows of a context that never made them."""
    c = _case(600, 5)
    other = _pushed(c.model.gpr()).device
    rng = np.random.default_rng(2)
    Xa, Xb = rng.uniform(-3, 3, (24, c.model.d)), rng.uniform(-3, 3, (9, c.model.d))
    for dev, cross in ((c.dev, True), (other, False)):
        dev.kb_reset()
        first, var_a = dev.kb_register(Xa)
        assert first == 0
        before = dev.kb_gram(5, 24)
        if cross:
            dev.loo()
            dev.leave_out([np.arange(40), [599, 1]])
            np.testing.assert_array_equal(dev.kb_gram(5, 24)[0], before[0])
        first, var_b = dev.kb_register(Xb)
        assert first == 24
        if cross:
            dev.loo(want=("var_y",))
        res = [var_a, var_b, *dev.kb_gram(30, 33), *dev.kb_gram(5, 33)]
        if cross:
            mine = res
    for a, b in zip(mine, res):
        np.testing.assert_array_equal(a, b)
    # and predict is what it was
    Xq = rng.uniform(-3, 3, (50, c.model.d))
    m0, s0 = other.predict(Xq, return_std=True)
    m1, s1 = c.dev.predict(Xq, return_std=True)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(s0, s1)


@pytest.mark.parametrize("i,N", [(2, 130), (6, 1100)])
def test_the_one_step_ahead_densities_sum_to_the_devices_lml(i, N):
    """sum_k log N(y_k; seq_mean_k, seq_var_y_k), taken back to transformed space, against gpry_lml at the same theta:
    1e-10 max(1, |LML|), the tolerance the suite holds the device's LML to (tests/test_lml_batch_gpu.py)."""
    c = _case(N, i)
    z = (c.gpr.y_train - c.out["seq_mean"]) / np.sqrt(c.out["seq_var_y"])
    total = float(np.sum(-0.5 * z * z - 0.5 * np.log(2 * np.pi * c.out["seq_var_y"] / c.y_std ** 2)))
    kid, theta = c.gpr._device_theta()
    lml = c.dev.lml(theta)[0]
    quad = float(z.dot(z))
    print(f"N={N}: sum of the one-step-ahead log densities {total:.15g}, gpry_lml {lml:.15g}, difference "
          f"{abs(total - lml):.2e} (bound {1e-10 * max(1.0, abs(lml)):.2e}); sum z^2 = {quad:.12g}, y_.alpha_ = "
          f"{float(c.y_.dot(c.a)):.12g}")
    assert abs(total - lml) <= 1e-10 * max(1.0, abs(lml))
    after = c.dev.loo()
    for k in OUTPUTS:
        np.testing.assert_array_equal(after[k], c.out[k])       # the objective's evaluation left the factor alone


def test_refusals_and_a_context_without_a_factor():
    from gpry_amd._lib import Device, GpryHipError
    c = _case(129, 4)
    dev = c.dev
    good = dev.leave_out([[0, 1]])
    for bad, word in (([[0, 1], []], "empty"), ([list(range(65))], "at most 64"), ([[0, 129]], "outside"), ([[-1, 2]], "outside"),
                      ([[3, 7, 3]], "more than once"), ([], "ngroups = 0")):
        with pytest.raises(GpryHipError, match=word):
            dev.leave_out(bad)
        np.testing.assert_array_equal(dev.leave_out([[0, 1]])["cov"][0], good["cov"][0])       # as usable as before
    assert dev.timing("loo")[1] >= 0
    dev.timing_reset()
    dev.loo()
    dev.leave_out([[5]])
    assert dev.timing("loo")[1] == 1 and dev.timing("leave_out")[1] == 1 and dev.timing("loo")[0] > 0
    fresh = Device(dev.device)
    try:
        for call in (fresh.loo, lambda: fresh.leave_out([[0]])):
            with pytest.raises(GpryHipError, match="no valid factor"):
                call()
        fresh.set_train(c.gpr.X_train_, c.gpr.y_train_, c.noise)
        fresh.set_theta(*c.gpr._device_theta())
        for call in (fresh.loo, lambda: fresh.leave_out([[0]])):
            with pytest.raises(GpryHipError, match="no valid factor"):
                call()
        assert fresh.factorize() == 0
        np.testing.assert_allclose(fresh.loo()["seq_var_y"] * c.y_std ** 2, c.out["seq_var_y"], rtol=1e-14)
    finally:
        fresh.close()
