"""The sweep of a pool whose sampler supplied y, or y and sigma_y (gpry_sweep_logexp_given; the reference's
mpi.compute_y_parallel, gpry/mpi.py:182-218): sigma is the ordinary sweep's bit for bit, y is the caller's, the pruned
sigma-only sweep gives the full one's records without a mean pass, masks follow predict_std (no trust-region gate), and
NORA.multi_add with such a sampler equals the reference's flow composed from the oracle."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gpry_oracle as orc
from test_given_y_cpu import oracle_given
from test_host_mirror_gpu import make_gpr
from test_sweep_prune_gpu import FIELDS, _theta_bench_like

pytestmark = pytest.mark.gpu


def _pair(bounds, X, y, kid, theta, **kw):
    """The device model and the oracle on the same data and theta."""
    theta = np.asarray(theta, dtype=float)
    gpr = make_gpr(bounds, kid, theta=theta, **kw)
    gpr.append_to_data(X, y, fit_gpr=False)
    gpr._ensure_factor()
    gpr._push_affine()
    ref = orc.OracleGPR(bounds, kernel_id=kid)
    ref.theta = theta.copy()
    ref.fitted = True
    fin = np.isfinite(y)
    ref.append_to_data(X[fin], y[fin], fit_gpr=False, fit_preprocessors=True)
    return gpr, ref


def _f7(tag):
    g = load_golden("multi_add")
    p = f"f7{tag}_"
    kid, M = int(g[p + "kid"]), int(g[p + "M"])
    N, d = g[p + "X"].shape
    bounds, X, y, Xc = orc.synthetic_like_goldens(N, d, M, int(g[p + "seed"]))
    return g, p, kid, bounds, X, y, Xc


def _config2():
    N, d, M = 4096, 16, 1_000_000
    bounds, X, y, Xc = orc.synthetic_problem(N, d, M)
    return orc.MATERN52, bounds, X, y, Xc, _theta_bench_like(d)


def _args(gpr):
    return orc.auto_zeta(gpr.d), gpr.y_max, gpr.noise_level


def _perturbed(y, seed=4):
    fin = np.isfinite(y)
    return y + 0.1 * np.std(y[fin]) * np.random.default_rng(seed).standard_normal(len(y))


def _check_sigma_only(gpr, ref, Xc, n_sub=2000):
    dev = gpr.device
    zeta, base, sn = _args(gpr)
    M = len(Xc)
    full = dev.sweep_logexp(Xc, zeta, base, sn)
    ft, fb = dev.sweep_topk(256)
    yg = _perturbed(full["y"])
    got = dev.sweep_logexp(None, zeta, base, sn, M=M, y_given=yg)
    assert got["n_nan"] == 0
    np.testing.assert_array_equal(got["sigma"], full["sigma"])
    np.testing.assert_array_equal(got["y"], yg)
    sub = np.sort(np.random.default_rng(5).choice(M, min(n_sub, M), replace=False))
    so = ref.predict_std(Xc[sub])
    np.testing.assert_allclose(got["sigma"][sub], so, rtol=1e-6, atol=1e-9)
    oa = orc.logexp_f(yg[sub], so, ref.y_max, ref.noise_level, zeta)
    np.testing.assert_allclose(got["acq"][sub], oa, rtol=1e-6, atol=1e-6)
    # the sweep's own y handed back: the ordinary sweep's acquisition and shortlist, bit for bit
    same = dev.sweep_logexp(None, zeta, base, sn, M=M, y_given=full["y"])
    np.testing.assert_array_equal(same["acq"], full["acq"])
    np.testing.assert_array_equal(same["sigma"], full["sigma"])
    st, sb = dev.sweep_topk(256)
    for f in FIELDS:
        np.testing.assert_array_equal(st[f], ft[f], err_msg=f)
    assert sb == fb
    return yg


def test_f7_sized_sigma_only_sweep():
    g, p, kid, bounds, X, y, Xc = _f7("b")
    gpr, ref = _pair(bounds, X, y, kid, g[p + "theta"])
    _check_sigma_only(gpr, ref, Xc)


@pytest.mark.timeout(900)
def test_config2_sigma_only_full_and_pruned():
    kid, bounds, X, y, Xc, theta = _config2()
    gpr, ref = _pair(bounds, X, y, kid, theta)
    dev = gpr.device
    M = len(Xc)
    yg = _check_sigma_only(gpr, ref, Xc, n_sub=1000)
    zeta, base, sn = _args(gpr)
    full = dev.sweep_logexp(None, zeta, base, sn, M=M, y_given=yg)
    ft, fb = dev.sweep_topk(256)
    dev.timing_reset()
    try:
        dev.set_option("sweep_prune", 1)
        try:
            out = dev.sweep_logexp(None, zeta, base, sn, M=M, want=(), y_given=yg)
        finally:
            dev.set_option("sweep_prune", 0)
        assert out["n_nan"] == 0
        # stage A built no panel and no mean: the bound kernel alone
        assert dev.timing("cross_build")[1] == 0 and dev.timing("sweep_mean")[1] == 0
        assert dev.timing("sweep_given_bound")[1] >= 1
    finally:
        dev.set_option("timing", 0)
    pt, pb = dev.sweep_topk(256)
    info = dev.sweep_prune_info()
    for f in FIELDS:
        np.testing.assert_array_equal(pt[f], ft[f], err_msg=f)
    assert pb >= fb, (pb, fb)
    assert info["pruned"] == 1 and info["completed"] == 0 and 0 < info["contracted"] < M, info
    print(f"sigma-only pruned, config2 size, theta = log[4, 0.3...]: contracted {info['contracted']} of {M}, "
          f"K' = {info['K_prime']}, survivors {info['survivors']}")
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(got[k], full[k], err_msg=k)
    assert dev.sweep_prune_info()["pruned"] == 0


def test_masks_follow_predict_std():
    """Classifier-inf rows: sigma 0, acq -inf.  Rows outside the trust region keep the caller's y, their sigma and a finite
    acquisition (predict_std has no trust-region gate) -- with the caller's mask and with the device gates."""
    from gpry_amd import _lib
    bounds, X, y, Xc = orc.synthetic_like_goldens(200, 4, 50000, seed=31)
    y = y.copy()
    y[X[:, 0] > 1.0] = -np.inf
    gpr, ref = _pair(bounds, X, y, 3, np.log(np.array([4.0, 0.3, 0.3, 0.3, 0.3])), account_for_inf="SVM",
                     inf_threshold="20s", trust_region_factor=1.5, random_state=1)
    dev = gpr.device
    zeta, base, sn = _args(gpr)
    host = gpr._masks(Xc, False, False)
    cls = (host & _lib.MASK_CLASSIFIED_INF) != 0
    trust = host == _lib.MASK_OUTSIDE_TRUST
    assert 100 < cls.sum() < len(Xc) - 100 and trust.sum() > 100
    yg = -np.abs(np.random.default_rng(6).standard_normal(len(Xc))) * 5.0
    dev.set_gates()
    out = dev.sweep_logexp(Xc, zeta, base, sn, mask=host, y_given=yg)
    np.testing.assert_array_equal(out["y"], yg)
    assert not out["sigma"][cls].any() and np.isneginf(out["acq"][cls]).all()
    assert np.isfinite(out["acq"][trust]).all() and (out["sigma"][trust] > 0).all()
    so = ref.predict_std(Xc)
    so[cls] = 0.0
    np.testing.assert_allclose(out["sigma"], so, rtol=1e-6, atol=1e-9)
    oa = orc.logexp_f(yg, so, ref.y_max, ref.noise_level, zeta)
    np.testing.assert_array_equal(np.isneginf(out["acq"]), np.isneginf(oa))
    np.testing.assert_allclose(out["acq"][~cls], oa[~cls], rtol=1e-6, atol=1e-6)
    # the device gates (which also set the trust bit): same values away from the decision boundary
    assert gpr._push_gates() is True
    dg = dev.sweep_logexp(Xc, zeta, base, sn, y_given=yg)
    dec = gpr.infinities_classifier._svc.decision_function(gpr.preprocessing_X.transform(Xc))
    clear = np.abs(dec) > 1e-9
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(dg[k][clear], out[k][clear], err_msg=k)
    dev.set_gates()


def test_both_given_is_the_acquisition_alone():
    g, p, kid, bounds, X, y, Xc = _f7("b")
    gpr, ref = _pair(bounds, X, y, kid, g[p + "theta"])
    dev = gpr.device
    zeta, base, sn = _args(gpr)
    M = len(Xc)
    rng = np.random.default_rng(7)
    yg = ref.predict(Xc) + rng.standard_normal(M)
    sg = ref.predict_std(Xc) * rng.uniform(0.5, 1.5, M)
    sg[:10] = 0.0
    mask = np.ones(M, np.uint8)                 # ignored
    out = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, y_given=yg, sigma_given=sg)
    oa = orc.logexp_f(yg, sg, ref.y_max, ref.noise_level, zeta)
    np.testing.assert_array_equal(out["y"], yg)
    np.testing.assert_array_equal(out["sigma"], sg)
    assert np.isneginf(out["acq"][:10]).all()
    np.testing.assert_allclose(out["acq"][10:], oa[10:], rtol=1e-13)
    top, bound = dev.sweep_topk(64)
    order = np.lexsort((-np.arange(M), -out["acq"]))
    np.testing.assert_array_equal(top["idx"], order[:64])
    np.testing.assert_array_equal(top["acq"], out["acq"][order[:64]])
    np.testing.assert_array_equal(top["y"], yg[order[:64]])
    np.testing.assert_array_equal(top["sigma"], sg[order[:64]])
    assert bound == out["acq"][order[64]]
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    np.testing.assert_array_equal(got["acq"], out["acq"])


def _given_nora(bounds, sample, **kw):
    from gpry_amd.gp_acquisition import NORA

    class GivenNORA(NORA):
        def do_MC_sample(self, gpr, bounds=None, rng=None, sampler=None):
            return sample

    return GivenNORA(bounds, sampler="uniform", verbose=0, **kw)


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("with_sigma", [False, True])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_multi_add_with_a_sampler_that_returns_y(tag, with_sigma, prune, devices):
    g, p, kid, bounds, X, y, Xc = _f7(tag)
    gpr, ref = _pair(bounds, X, y, kid, g[p + "theta"])
    npts = len(g[p + "acq_cond"]) - 1
    M = len(Xc)
    rng = np.random.default_rng(8)
    yg = ref.predict(Xc) + 0.5 * rng.standard_normal(M)
    sg = ref.predict_std(Xc) * 0.9 if with_sigma else None
    w = rng.uniform(0.5, 1.0, M)
    acq = _given_nora(bounds, (Xc, yg, sg, w), mc_every=2, devices=devices, exact_prune=prune, shortlist_size=32)
    n0 = gpr.n_eval
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    Xo, yo, ao, so, _ = oracle_given(ref, Xc, yg, sg, npts, zeta=acq.acq_func.zeta)
    np.testing.assert_array_equal(Xp, Xo)
    np.testing.assert_allclose(yp, yo, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(ap, ao, rtol=1e-7, atol=1e-7)
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert ys is yg and Xs is Xc and ws is w
    if with_sigma:
        assert ss is sg
    else:
        np.testing.assert_allclose(ss, so, rtol=1e-6, atol=1e-9)
        assert gpr.n_eval - n0 >= M
    # second call of mc_every = 2: re-weighted against the caller's y
    y_new = g[p + "y_new"][:len(Xp)]
    gpr.append_to_data(Xp, y_new, fit_gpr=False)
    ref.append_to_data(Xp, y_new, fit_gpr=False, fit_preprocessors=True)
    acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    assert acq.is_last_MC_reweighted
    with np.errstate(all="ignore"):
        wn = w * np.exp(ref.predict(Xc) - yg)
    wn /= wn.max()
    keep = wn != 0
    Xr, yr, sr, wr = acq.last_MC_sample(warn_reweight=False)
    np.testing.assert_array_equal(Xr, Xc[keep])
    np.testing.assert_allclose(wr, wn[keep], rtol=1e-6, atol=1e-12)


def test_nan_in_the_samplers_y_raises():
    g, p, kid, bounds, X, y, Xc = _f7("a")
    gpr, ref = _pair(bounds, X, y, kid, g[p + "theta"])
    yg = ref.predict(Xc)
    yg[17] = np.nan
    acq = _given_nora(bounds, (Xc, yg, None, None), devices=[0])
    with pytest.raises(ValueError, match="not a number"):
        acq.multi_add(gpr, n_points=2, rng=np.random.default_rng(0))
