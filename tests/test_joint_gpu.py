"""Joint posterior covariance and joint draws of the surrogate on the device (gpry_amd/csrc/joint.hip, Device.predict_cov /
sample_joint, GaussianProcessRegressor.predict(return_cov=True) / sample_y, gpry_amd/mc.py: surrogate_spread): the
covariance against the float64 closed form of tests/tools/joint_numpy.py at every (builder, tile edge, k-split, kernel id),
with the closed form's own error against extended precision printed beside it; an entry's bits depend on the model and
the two points alone, a draw's on the seed and its index; the Cholesky factor and the product Z L_c^T each against their
backward-error bounds, the variates against the numpy Philox restatement; the draws' moments; the jitter ladder; the
gates; the refusals; and the propagation end to end on a 12-point and a 200-point surrogate of the same posterior."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed
from test_nested_gpu import _fitted, _gauss_ll, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import joint_numpy as jn  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_CACHE = {}


def _model(d, kid, N, affine=True, **kw):
    """(model, pushed gpr, oracle), one of each per case of the file."""
    key = (d, kid, N, affine, tuple(sorted(kw.items())))
    if key not in _CACHE:
        model = sw.Model(d, kid, N, affine=affine, seed=N + d, **kw)
        gpr = _pushed(model.gpr())
        _CACHE[key] = (model, gpr, model.oracle(gpr))
    return _CACHE[key]


def _unit(model, gpr):
    """C y_std^2: the unit of the bounds and of the jitter."""
    return float(np.exp(model.theta[0])) * float(gpr._y_affine()[1]) ** 2


def _points(gpr, m, seed, n_train=None):
    rng = np.random.default_rng(seed)
    d = gpr.X_train.shape[1]
    n_train = min((m + 1) // 2, len(gpr.X_train)) if n_train is None else n_train      # (every training row at most once)
    X = rng.uniform(-3.0, 3.0, (m, d))
    X[:n_train] = gpr.X_train[rng.choice(len(gpr.X_train), n_train, replace=False)]
    return np.ascontiguousarray(X)


# every N with every m; d, the kernel id and the affine maps go round; Matern 1/2 once
COV_CASES = [(N, m, (2, 9, 17, 32)[(i + j) % 4], (sw.RBF, sw.M32, sw.M52)[(i + 2 * j) % 3], (i + j) % 2 == 0)
             for i, N in enumerate((100, 1100, 2500)) for j, m in enumerate((1, 127, 129, 513))] + [(1100, 129, 9, sw.M12, True)]


@pytest.mark.parametrize("N,m,d,kid,affine", COV_CASES)
def test_covariance_against_the_closed_form(N, m, d, kid, affine):
    """Half of the points (all the training rows, where there are fewer) are training rows, where K** - U^T U cancels
    worst.  Bound: 1e-6 C y_std^2, the project's specification of the posterior variance; the
    diagonal against gpry_predict's std^2 the same."""
    model, gpr, ref = _model(d, kid, N, affine)
    X = _points(gpr, m, 7 * m + d)
    out = gpr.device.predict_cov(X)
    S = jn.cov_of_oracle(ref, X)
    unit = _unit(model, gpr)
    err = float(np.max(np.abs(out["cov"] - S)))
    sub = np.unique(np.concatenate([np.arange(min(m, 3)), np.arange(max(m - 3, 0), m)]))        # training rows and others
    Sl = jn.cov_of_oracle(ref, X[sub], dtype=np.longdouble)
    err_ref = float(np.max(np.abs(np.asarray(Sl - S[np.ix_(sub, sub)], dtype=float))))
    mean, std = gpr.device.predict(X, return_std=True)
    err_diag = float(np.max(np.abs(np.diag(out["cov"]) - std ** 2)))
    print(f"N={N} m={m} d={d} kid={kid} affine={affine}: max|Sigma_dev - Sigma_ref| = {err / unit:.3e} C y_std^2 "
          f"(bound 1e-6), float64 closed form against longdouble {err_ref / unit:.3e}, diagonal against predict's std^2 "
          f"{err_diag / unit:.3e}, device {out['device_ms']:.3f} ms")
    assert err <= 1e-6 * unit
    assert err_diag <= 1e-6 * unit
    np.testing.assert_array_equal(out["cov"], out["cov"].T)
    assert np.max(np.abs(out["mean"] - mean)) <= model.tol()


def test_an_entry_depends_on_the_model_and_its_two_points_alone():
    """Sigma_ab alone as a 2-point batch (small builder), inside a 513-point batch (large builder) at any position, after
    a permutation and on a second context; N = 2500: both products run split over k."""
    model = sw.Model(9, sw.M52, 2500, seed=2)
    gpr, gpr2 = _pushed(model.gpr()), _pushed(model.gpr())
    assert gpr2.device is not gpr.device
    X = _points(gpr, 513, 5, n_train=100)
    a, b = gpr.device.predict_cov(X), gpr2.device.predict_cov(X)
    np.testing.assert_array_equal(a["cov"], b["cov"])
    np.testing.assert_array_equal(a["mean"], b["mean"])
    perm = np.random.default_rng(1).permutation(513)
    p = gpr.device.predict_cov(np.ascontiguousarray(X[perm]))
    np.testing.assert_array_equal(p["cov"], a["cov"][np.ix_(perm, perm)])
    for i, j in ((0, 1), (100, 400), (512, 3), (256, 128), (511, 512)):
        two = gpr.device.predict_cov(np.ascontiguousarray(X[[i, j]]))
        np.testing.assert_array_equal(two["cov"], a["cov"][np.ix_([i, j], [i, j])], err_msg=f"{i} {j}")
    assert np.all(np.isfinite(a["cov"]))


def test_a_draw_depends_on_the_seed_and_its_index_alone():
    model, gpr, _ = _model(9, sw.M52, 1100)
    X = _points(gpr, 129, 3, n_train=10)
    Y = {S: gpr.device.sample_joint(X, S, 99)["Y"] for S in (1, 7, 300)}
    np.testing.assert_array_equal(Y[300][:7], Y[7])
    np.testing.assert_array_equal(Y[300][:1], Y[1])
    assert not np.array_equal(Y[7], gpr.device.sample_joint(X, 7, 100)["Y"])
    assert np.all(np.isfinite(Y[300]))


@pytest.mark.parametrize("m,S,N,d", [(1, 1, 100, 2), (64, 33, 100, 2), (129, 256, 1100, 9), (1000, 33, 1100, 9),
                                     (4096, 1, 300, 9)])
def test_the_factor_and_the_product_each_alone(m, S, N, d):
    """L_c L_c^T against Sigma_dev + eps C y_std^2 I within 8 (m + 1) u max diag (the Cholesky backward-error bound); Y
    against mu + Z L_c^T recomputed in numpy (float64, so the final addition of mu rounds as the device's does) from the
    device's own Z, L_c and mu within the dot-product bound 4 m u (|Z| |L_c|^T) entrywise; Z against the numpy Philox
    restatement within the tolerance the sampler-walk tests hold the device's normals to (sampler_walk.POS_TOL).
    m = 4096 on N = 300: the panel chain's segment boundary above 3584 rows.  No clip: the finalised mean is mu.
    Measured: the product's error is at most 0.003 of its bound, the factor's at most 0.007 of its own."""
    model, gpr, _ = _model(d, sw.M52, N, clip_factor=None)
    assert np.isinf(gpr._clip_hi())
    X = _points(gpr, m, m + S, n_train=0)
    unit = _unit(model, gpr)
    cov = gpr.device.predict_cov(X)["cov"]
    res = gpr.device.sample_joint(X, S, 1234, want_Z=True, want_Lc=True)
    L, Z, mu, eps = res["Lc"], res["Z"], res["mean"], res["jitter_used"]
    assert eps in list(jn.ladder(None))
    np.testing.assert_array_equal(L, np.tril(L))
    A = cov + eps * unit * np.eye(m)
    e_chol = float(np.max(np.abs(L @ L.T - A)))
    b_chol = 8 * (m + 1) * U * float(np.max(np.diag(A)))
    e_z = float(np.max(np.abs(Z - jn.normals(1234, S, m))))
    R = mu[None, :] + Z @ L.T
    bound = 4 * m * U * (np.abs(Z) @ np.abs(L).T)
    ratio = float(np.max(np.abs(res["Y"] - R) / bound))
    print(f"m={m} S={S} N={N}: eps = {eps:g}, |L L^T - A|max = {e_chol:.3e} (bound {b_chol:.3e}), |Y - (mu + Z L^T)| / bound "
          f"= {ratio:.3f}, |Z - numpy|max = {e_z:.3e} (tolerance {sw.POS_TOL:.1e}), device {res['device_ms']:.3f} ms")
    assert e_chol <= b_chol
    assert ratio <= 1.0
    assert e_z <= sw.POS_TOL


STAT_SEED = 1      # chosen so that the numpy stand-in with the same Philox stream passes the 27 conditions below on the CPU


def _stat_case():
    model, gpr, ref = _model(2, sw.M52, 100)
    X = np.array([[-3.5, -3.5], [3.5, -3.0], [-3.0, 3.5], [3.5, 3.5], [0.0, -3.8], [3.9, 0.5]])
    return model, gpr, ref, X


def _stat_check(Y, mu, S):
    n = len(Y)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / n)
    dev_c = np.abs(np.cov(Y.T, bias=True) - S) / se
    dev_m = np.abs(Y.mean(axis=0) - mu) / np.sqrt(np.diag(S) / n)
    return float(dev_c.max()), float(dev_m.max())


def test_the_moments_of_the_draws():
    """m = 6 well-separated points, S = 8192: every entry of the sample covariance within 5 standard errors of Sigma
    (SE_ij = sqrt((S_ii S_jj + S_ij^2) / S)), every sample mean within 5 sqrt(S_ii / S) of mu: 21 + 6 statistics.  Five
    standard errors over 27 statistics is a condition, not a measurement: STAT_SEED was chosen so that the numpy stand-in
    (tests/tools/joint_numpy.py, the same Philox stream) passes it on the CPU."""
    model, gpr, ref, X = _stat_case()
    cov = gpr.device.predict_cov(X)
    res = gpr.device.sample_joint(X, 8192, STAT_SEED)
    assert np.all(np.diag(cov["cov"]) > 1e-3 * _unit(model, gpr))
    dc, dm = _stat_check(res["Y"], cov["mean"], cov["cov"])
    print(f"largest deviation of a covariance entry {dc:.2f} SE, of a mean {dm:.2f} SE")
    assert dc <= 5.0 and dm <= 5.0


def test_the_jitter_ladder():
    model, gpr, _ = _model(2, sw.M52, 100)
    unit, y_std = _unit(model, gpr), float(gpr._y_affine()[1])
    X = _points(gpr, 40, 11, n_train=5)
    X[17] = X[4]                                    # an exact duplicate pair
    res = gpr.device.sample_joint(X, 33, 5, jitter=0.0)
    eps = res["jitter_used"]
    assert eps > 0 and eps in list(jn.ladder(0.0))
    assert np.all(np.isfinite(res["Y"]))
    gap = float(np.max(np.abs(res["Y"][:, 17] - res["Y"][:, 4])))
    print(f"duplicate pair: jitter_used = {eps:g}, largest gap between the two columns {gap:.3e} "
          f"(bound {10 * np.sqrt(eps * np.exp(model.theta[0])) * y_std:.3e})")
    assert gap <= 10 * np.sqrt(eps * np.exp(model.theta[0])) * y_std
    good = gpr.device.sample_joint(_stat_case()[3], 33, 5, jitter=0.0)
    assert good["jitter_used"] == 0.0 and np.all(np.isfinite(good["Y"]))
    assert gpr.device.sample_joint(X, 3, 5, jitter=1e-6)["jitter_used"] == 1e-6


def test_the_gates():
    """Rejected rows: a zero row and column and -inf in every draw; the other rows' Sigma and draws are the bits of a call
    without the rejected rows (which stand last, so that every row keeps its variates); a row outside the trust region
    alone has mean -inf and its Sigma untouched."""
    from gpry_amd._lib import MASK_CLASSIFIED_INF, MASK_OUTSIDE_TRUST
    gpr, bounds = _svm_model()
    _pushed(gpr)
    rng = np.random.default_rng(1)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (64, 3))
    X[:8, 0] = rng.uniform(2.0, 3.9, 8)                     # the classifier's rejected side
    tb = np.asarray(gpr.trust_bounds)
    X[8:12] = np.clip(X[8:12], tb[:, 0], tb[:, 1])
    X[8:12, 0] = -1.0
    X[8:12, 1] = tb[1, 1] + 0.05 * np.arange(1, 5)          # beyond the trust box in one coordinate
    bits = gpr._masks(X, False, False)
    dead = (bits & MASK_CLASSIFIED_INF) != 0
    trust_only = bits == MASK_OUTSIDE_TRUST
    assert dead[:8].all() and trust_only.any() and (bits == 0).sum() >= 16
    order = np.argsort(dead, kind="stable")
    X, bits, dead, trust_only = np.ascontiguousarray(X[order]), bits[order], dead[order], trust_only[order]
    nlive = int((~dead).sum())
    on = gpr.device.predict_cov(X)
    draws = gpr.device.sample_joint(X, 33, 8)
    np.testing.assert_array_equal(np.isneginf(on["mean"]), bits != 0)
    assert np.all(on["cov"][dead, :] == 0.0) and np.all(on["cov"][:, dead] == 0.0)
    assert np.all(np.isneginf(draws["Y"][:, dead])) and np.all(np.isfinite(draws["Y"][:, ~dead]))
    assert np.all(np.diag(on["cov"])[trust_only] > 0.0)
    live = gpr.device.predict_cov(X[:nlive])
    np.testing.assert_array_equal(live["cov"], on["cov"][:nlive, :nlive])
    np.testing.assert_array_equal(live["mean"], on["mean"][:nlive])
    np.testing.assert_array_equal(gpr.device.sample_joint(X[:nlive], 33, 8)["Y"], draws["Y"][:, :nlive])
    # without the gates: the rows that were not rejected keep their Sigma (the trust region changes the mean only)
    gpr.device.set_gates()
    off = gpr.device.predict_cov(X)
    assert np.all(np.isfinite(off["mean"]))
    np.testing.assert_array_equal(off["cov"][:nlive, :nlive], on["cov"][:nlive, :nlive])
    # a caller's mask does what the device gates do
    mk = gpr.device.predict_cov(X, mask=bits)
    np.testing.assert_array_equal(mk["cov"], on["cov"])
    np.testing.assert_array_equal(mk["mean"], on["mean"])


def test_bad_arguments_are_refused_and_the_context_stays_usable():
    from gpry_amd._lib import Device, GpryHipError
    model, gpr, _ = _model(2, sw.M52, 100)
    dev = gpr.device
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    X = np.zeros((4097, 2))
    X[:, 0] = np.linspace(-3, 3, 4097)
    mean, cov, Y = np.empty(4097), np.empty((4, 4)), np.empty((3, 4))
    eps, info = ctypes.c_double(0.0), ctypes.c_int(0)

    def pc(X=X, m=4, cov=cov):
        rc = dev._lib.gpry_predict_cov(dev._h, vp(X), m, None, vp(mean), vp(cov), None)
        return rc, dev._lib.gpry_last_error(dev._h).decode()

    def sj(X=X, m=4, S=3, Y=Y, jitter=-1.0):
        rc = dev._lib.gpry_sample_joint(dev._h, vp(X), m, None, S, 1, jitter, vp(mean), vp(Y), None, None,
                                        ctypes.byref(info), ctypes.byref(eps), None)
        return rc, dev._lib.gpry_last_error(dev._h).decode()

    nan = X[:4].copy()
    nan[2, 1] = np.nan
    for call, name in ((pc, "gpry_predict_cov"), (sj, "gpry_sample_joint")):
        assert call()[0] == 0
        for kw, word in ((dict(m=0), "m = 0"), (dict(m=4097), "m = 4097"), (dict(X=nan), "not finite"),
                         (dict(X=None), "NULL")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and name in msg, (kw, rc, msg)
        assert call()[0] == 0                        # the context is as usable as before
    rc, msg = pc(cov=None)
    assert rc == -1 and "cov is NULL" in msg
    for kw, word in ((dict(S=0), "S = 0"), (dict(S=65537), "S = 65537"), (dict(Y=None), "Y is NULL"),
                     (dict(jitter=float("nan")), "jitter")):
        rc, msg = sj(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert sj()[0] == 0 and pc()[0] == 0
    with pytest.raises(GpryHipError, match="m = 4097"):
        dev.predict_cov(X)
    with pytest.raises(GpryHipError, match="S = 0"):
        dev.sample_joint(X[:4], 0, 1)
    with pytest.raises(ValueError):
        dev.predict_cov(np.zeros((2, 3)))
    fresh = Device(dev.device)               # no factor yet
    fresh.d = 2
    for call in (lambda: fresh.predict_cov(X[:4]), lambda: fresh.sample_joint(X[:4], 2, 1)):
        with pytest.raises(GpryHipError, match="training set|model|factor"):
            call()
    fresh.close()
    assert pc()[0] == 0


@pytest.mark.timeout(900)
def test_the_spread_shrinks_with_the_training_set_and_the_class_agrees_with_the_device():
    from gpry_amd.mc import mc_sample_from_gp, surrogate_spread
    out = {}
    for N in (12, 200):
        gpr, bounds = _fitted(_gauss_ll(2), 2, N, seed=3)
        X, y, w = mc_sample_from_gp(gpr, bounds=bounds, sampler="mcmc", seed=5, sampler_options={"max_samples": 40000})
        last = mc_sample_from_gp.last_result
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (the 12-point surrogate may well trip the ESS warning)
            out[N] = surrogate_spread(gpr, X, y, w, n_draws=128, seed=6, max_points=1024)
        assert mc_sample_from_gp.last_result is last
        print(N, out[N])
    for r in out.values():
        assert r.logZ_std > 0 and np.all(r.mean_shift_sigma > 0) and r.n_points <= 1024
    assert out[200].logZ_std < out[12].logZ_std
    assert np.all(out[200].mean_shift_sigma < out[12].mean_shift_sigma)
    # the class against the Device calls
    Xq = np.ascontiguousarray(X[:50])
    n0 = gpr.n_eval
    mean, cov = gpr.predict(Xq, return_cov=True)
    dv = gpr.device.predict_cov(Xq)
    np.testing.assert_array_equal(cov, dv["cov"])
    np.testing.assert_array_equal(mean, dv["mean"])
    Y = gpr.sample_y(Xq, n_samples=9, random_state=4)
    assert Y.shape == (50, 9) and gpr.n_eval == n0 + 100
    np.testing.assert_array_equal(Y, gpr.device.sample_joint(Xq, 9, 4)["Y"].T)
    assert type(gpr).sample_y.last_result["jitter_used"] >= 1e-10
    with pytest.raises(ValueError, match="return_cov"):
        gpr.predict(Xq[:1], return_cov=True, return_std=True)
