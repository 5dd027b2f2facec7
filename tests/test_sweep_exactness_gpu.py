"""Deterministic edges of the pruned sweep (option "sweep_prune") and of the sigma-only sweep (sampler-supplied y): a block
of far candidates whose acquisitions tie bit for bit with their bounds at the K-th place, a noise floor above the prior
variance, pools where every candidate is masked or gated, calls interleaved with predict and a refit, and N <= 128 (one row
tile) for every kernel.  Pruned and full records are equal bit for bit, the pruned bound is >= the full one, and the
fetched arrays are the full sweep's."""
import numpy as np
import pytest

from gpry_amd import _lib
from oracle import gpry_oracle as orc

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "acq", "y", "sigma")


@pytest.fixture(scope="module")
def dev():
    d = _lib.Device(0)
    yield d
    d.close()


def _model(N, d, kid, theta, seed=0, noise=1e-2):
    rng = np.random.default_rng(seed)
    bounds = np.array([[-5.0, 5.0]] * d)
    X = rng.uniform(-5, 5, (N, d))
    y = -0.5 * (X ** 2).sum(1)
    m = orc.OracleGPR(bounds, kernel_id=kid, noise_level=noise)
    m.theta = np.asarray(theta, dtype=float)
    m.fitted = True
    m.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    return m, bounds, X


def _load(dev, m):
    dev.set_train(m.X_train_, m.y_train_, m.alpha)
    dev.set_theta(m.kernel_id, m.theta)
    dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
    assert dev.factorize() == 0


def _sweep(dev, X, M, args, prune, mask=None, y_given=None):
    dev.set_option("sweep_prune", int(prune))
    try:
        return dev.sweep_logexp(X, *args, mask=mask, M=M, want=() if prune else ("y", "sigma", "acq"), y_given=y_given)
    finally:
        dev.set_option("sweep_prune", 0)


def _same(a, b):
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


def _compare(dev, Xc, args, calls, mask=None, y_given=None):
    """calls: (K, exclusions) asked of the full sweep, then of a pruned sweep of the same resident pool; returns the full
    arrays and the prune info after each pruned call."""
    M = len(Xc)
    full = _sweep(dev, Xc, M, args, False, mask, y_given)
    ref = [dev.sweep_topk(K, exclude=ex) for K, ex in calls]
    out = _sweep(dev, None, M, args, True, mask, y_given)
    assert out["n_nan"] == full["n_nan"]
    infos = []
    for (K, ex), (ft, fb) in zip(calls, ref):
        pt, pb = dev.sweep_topk(K, exclude=ex)
        infos.append(dev.sweep_prune_info())
        _same(pt, ft)
        assert pb >= fb, (K, pb, fb, infos[-1])
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(got[k], full[k], err_msg=k)
    return full, ref, infos


def test_tie_pool_of_far_candidates_at_the_kth_place(dev):
    """3000 far candidates (k* = 0: y = y_mean, sigma the prior's, the acquisition equal to its bound bit for bit) above
    36000 near ones whose bounds are all lower.  Round 1 contracts the 1024 far rows of highest index; a shortlist of 1024
    then answers from them, and its bound is the next far row's bound -- which must be the full sweep's value.  1025 needs
    the next round.  Both paths against the oracle's ordering (acq desc, idx desc)."""
    d = 3
    m, bounds, X = _model(300, d, orc.MATERN52, np.log([1.0, 0.3, 0.3, 0.3]))     # C = exp(0) = 1 on host and device
    _load(dev, m)
    y_mean, y_std = m.pre_y.mean_, m.pre_y.std_
    sp = np.sqrt(1.0) * y_std                            # the prior sigma
    sn = np.sqrt(0.9) * sp                               # (amplifies a one-ulp change of the prior variance tenfold)
    args = (orc.auto_zeta(d), y_mean, sn)                # baseline = y_mean: the far rows' linear term is 0 exactly
    # a bound one ulp of C below the prior's would show in the far rows' acquisition
    lo = orc.logexp_f(y_mean, np.sqrt(1.0 - 2.0 ** -52) * y_std, y_mean, sn, args[0])
    assert lo < orc.logexp_f(y_mean, sp, y_mean, sn, args[0])
    rng = np.random.default_rng(3)
    n_near = 36000
    cand = rng.uniform(-5, 5, (100000, d))
    yc = dev.sweep_logexp(cand, *args, want=("y",))["y"]
    near = cand[yc < y_mean - 1e-3 * y_std][:n_near]      # bound below the far rows' by far more than an ulp
    assert len(near) == n_near
    far = 5.0 + 1e4 + rng.uniform(0, 10, (3000, d))
    Xc = np.concatenate([near, far])
    M = len(Xc)
    full = dev.sweep_logexp(Xc, *args)
    a = full["acq"]
    a_far = a[n_near:]
    assert np.all(a_far == a_far[0]) and np.isfinite(a_far[0]) and not (a[:n_near] >= a_far[0]).any()
    np.testing.assert_array_equal(full["sigma"][n_near:], full["sigma"][n_near])
    np.testing.assert_array_equal(full["y"][n_near:], y_mean)
    ex = np.arange(M - 100, M)[::7]
    calls = [(1, None), (1024, None), (1025, None), (1500, ex), (2999, None), (3001, ex)]
    full, ref, infos = _compare(dev, Xc, args, calls)
    assert infos[0]["rounds"] == 1 and infos[1]["rounds"] == 1 and infos[0]["contracted"] == 1024, infos[:2]
    assert infos[2]["rounds"] >= 2 and infos[2]["completed"] == 0, infos[2]
    # the oracle: every far row at one value, the shortlist their indices descending
    ro, so = m.predict(Xc[[0, M - 1]], return_std=True)
    np.testing.assert_allclose(so[1], full["sigma"][M - 1], rtol=1e-12)
    for (K, exl), (top, bound) in zip(calls, ref):
        keep = np.setdiff1d(np.arange(n_near, M), exl if exl is not None else [])[::-1]
        np.testing.assert_array_equal(top["idx"][:min(K, len(keep))], keep[:K])
        assert bound == a_far[0] or K >= len(keep)


@pytest.mark.parametrize("given", [False, True])
def test_noise_floor_above_the_prior_variance_gives_minus_inf_everywhere(dev, given):
    m, bounds, X = _model(500, 4, orc.MATERN32, np.log([2.0, 0.4, 0.4, 0.4, 0.4]))
    _load(dev, m)
    sp = np.sqrt(2.0) * m.pre_y.std_
    Xc = np.random.default_rng(1).uniform(-6, 6, (30000, 4))
    yg = np.random.default_rng(2).normal(m.y_max, 1.0, len(Xc)) if given else None
    for sn in (sp * (1 + 1e-12), 3.0 * sp):
        args = (0.3, m.y_max, sn)
        full, ref, infos = _compare(dev, Xc, args, [(16, None), (300, np.arange(0, 30000, 97))], y_given=yg)
        assert np.isneginf(full["acq"]).all()
        assert np.isneginf(ref[0][0]["acq"]).all() and len(ref[0][0]) == 16


@pytest.mark.parametrize("how", ["mask_classified", "mask_mixed", "gates_svm", "gates_trust"])
@pytest.mark.parametrize("given", [False, True])
def test_every_candidate_masked_or_gated(dev, how, given):
    """Every acquisition -inf (sigma 0 where the classifier bit is set) with K > 0, on both paths.  Their bounds are -inf
    as well, so the pruned sweep answers in round 1 without completing.  (A sigma-only pool outside the trust region
    keeps its sigma and a finite acquisition: predict_std has no trust-region gate.)"""
    d = 4
    m, bounds, X = _model(700, d, orc.MATERN52, np.log([2.0, 0.4, 0.4, 0.4, 0.4]))
    _load(dev, m)
    M = 20000
    Xc = np.random.default_rng(5).uniform(-5, 5, (M, d))
    mask = None
    try:
        if how == "mask_classified":
            mask = np.full(M, _lib.MASK_CLASSIFIED_INF, np.uint8)
        elif how == "mask_mixed":
            mask = np.where(np.arange(M) % 3 == 0, _lib.MASK_OUTSIDE_TRUST,
                            _lib.MASK_CLASSIFIED_INF | (np.arange(M) % 2) * _lib.MASK_OUTSIDE_TRUST).astype(np.uint8)
        elif how == "gates_svm":        # one support vector, decision -10 everywhere: all classified infinite
            dev.set_gates(sv=np.full((1, d), 0.5), coef=np.array([1e-3]), gamma=1.0, intercept=-10.0)
        else:                           # a trust box no candidate is in
            dev.set_gates(trust_bounds=np.array([[6.0, 7.0]] * d))
        yg = np.random.default_rng(6).normal(m.y_max, 2.0, M) if given else None
        args = (orc.auto_zeta(d), m.y_max, m.noise_level)
        full, ref, infos = _compare(dev, Xc, args, [(16, None), (256, np.arange(0, M, 13))], mask=mask, y_given=yg)
    finally:
        dev.set_gates()
    cls = (mask & _lib.MASK_CLASSIFIED_INF) != 0 if mask is not None else np.full(M, how == "gates_svm")
    if given:
        np.testing.assert_array_equal(full["y"], yg)
        assert np.isneginf(full["acq"][cls]).all() and not full["sigma"][cls].any()
        assert (full["sigma"][~cls] > 0).all()
    else:
        assert np.isneginf(full["y"]).all() and np.isneginf(full["acq"]).all()
        assert not full["sigma"][cls].any() and (full["sigma"][~cls] > 0).all()
    if cls.all() or not given:
        assert np.isneginf(ref[0][0]["acq"]).all() and len(ref[0][0]) == 16
        assert infos[0]["rounds"] == 1 and infos[0]["completed"] == 0, infos[0]


def test_interleaved_predict_and_refit_keep_the_sweeps_model(dev):
    """pruned sweep -> predict(return_std) of five points (the small panel form) -> a refit with more rows (Np 256 -> 384)
    and another theta -> sweep_topk and sweep_fetch: the full sweep's records and arrays of the OLD model."""
    d = 5
    m, bounds, X = _model(250, d, orc.RBF, np.log([3.0] + [0.35] * d))
    _load(dev, m)
    Xc = np.random.default_rng(8).uniform(-5.2, 5.2, (60000, d))
    Xc[:40] = X[:40]
    args = (orc.auto_zeta(d), m.y_max, m.noise_level)
    M = len(Xc)
    full = _sweep(dev, Xc, M, args, False)
    form = dev.sweep_info()["panel_form"]
    ref = [dev.sweep_topk(K, exclude=ex) for K, ex in ((64, None), (1024, np.arange(0, 2000, 5)))]
    _sweep(dev, None, M, args, True)
    assert dev.sweep_info()["panel_form"] == form
    mu, sd = dev.predict(Xc[:5], return_std=True)
    assert dev.sweep_info()["panel_form"] == "small"
    rm, rs = m.predict(Xc[:5], return_std=True)
    np.testing.assert_allclose(mu, rm, rtol=0, atol=1e-8 * max(1.0, np.abs(m.y_train).max()))
    m2, _, _ = _model(300, d, orc.RBF, np.log([1.5] + [0.6] * d), seed=9)
    _load(dev, m2)
    for (K, ex), (ft, fb) in zip(((64, None), (1024, np.arange(0, 2000, 5))), ref):
        pt, pb = dev.sweep_topk(K, exclude=ex)
        _same(pt, ft)
        assert pb >= fb
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(got[k], full[k], err_msg=k)
    # and the refitted model sweeps as itself afterwards
    new = dev.sweep_logexp(Xc[:3000], orc.auto_zeta(d), m2.y_max, m2.noise_level, want=("y",))
    np.testing.assert_allclose(new["y"], m2.predict(Xc[:3000]), rtol=1e-8, atol=1e-8 * max(1.0, np.abs(m2.y_train).max()))


@pytest.mark.parametrize("kid", [orc.RBF, orc.MATERN12, orc.MATERN32, orc.MATERN52])
@pytest.mark.parametrize("N", [17, 128])
def test_pruned_sweep_with_one_row_tile(dev, kid, N):
    """N <= 128: Np = 128, one row tile, for every kernel; ordinary and sigma-only, against the oracle too."""
    d = 6
    m, bounds, X = _model(N, d, kid, np.log([2.0] + [0.5] * d), seed=N + kid)
    _load(dev, m)
    rng = np.random.default_rng(kid)
    Xc = rng.uniform(-5.5, 5.5, (50000, d))
    Xc[:N] = X
    args = (orc.auto_zeta(d), m.y_max, m.noise_level)
    calls = [(16, None), (256, np.arange(0, 50000, 11)), (5000, None)]
    full, ref, infos = _compare(dev, Xc, args, calls)
    sub = np.unique(np.concatenate([ref[1][0]["idx"], rng.choice(len(Xc), 500, replace=False)]))
    rm, rs = m.predict(Xc[sub], return_std=True)
    C = 2.0 * m.pre_y.std_ ** 2
    assert np.max(np.abs(full["y"][sub] - rm)) <= 1e-8 * max(1.0, np.abs(m.y_train).max())
    assert np.max(np.abs(full["sigma"][sub] ** 2 - rs ** 2)) <= 1e-9 * C
    yg = full["y"] + rng.normal(0, 0.2 * m.pre_y.std_, len(Xc))
    g, _, _ = _compare(dev, Xc, args, calls, y_given=yg)
    np.testing.assert_array_equal(g["sigma"], full["sigma"])


def test_completion_after_a_model_of_fewer_dimensions():
    """Regression: the gathered rows of a compact evaluation (sweep.hip: prune_eval, dXg) were sized in rows of the model that
    first needed them.  A completion at d = 3 that gathered ~38000 rows, then one at d = 8 of ~19000 rows, wrote past the
    buffer.  Own context, so that the d = 3 completion is the first one made on it."""
    dev = _lib.Device(0)
    try:
        for d, M in ((3, 40000), (8, 20000)):
            m, bounds, X = _model(200, d, orc.MATERN52, np.log([2.0] + [0.4] * d), seed=d)
            _load(dev, m)
            Xc = np.random.default_rng(d).uniform(-5, 5, (M, d))
            full, ref, infos = _compare(dev, Xc, (orc.auto_zeta(d), m.y_max, m.noise_level), [(8, None)])
            assert infos[0]["completed"] == 0
    finally:
        dev.close()
