"""``C * (RBF | Matern) + WhiteKernel`` on the device (GPRY_KERNEL_WHITE): a model (a, w) -- per-point noise a, fitted
noise level w -- against today's model with alpha = a + w (bit for bit where the arithmetic is shared), against golden
vectors of the reference (tests/golden/white_noise.npz) and against the numpy closed form (tests/tools/white_model.py).
Tolerances are those of test_hip_parity.py: kernel values 1e-13, LML 1e-10, gradient 1e-7 of its largest entry, mean
1e-8 / 1e-9, std 1e-6 / 1e-9 (variance 1e-9 of the prior variance), acquisition 1e-6.
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import white_model as wm  # noqa: E402
from oracle import gpry_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

W = 0x10


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-300))


def _device():
    from gpry_amd import _lib
    return _lib.Device(0)


@pytest.fixture(scope="module")
def dev():
    d = _device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def g():
    return load_golden("white_noise")


def problem(N, d, seed, log_w=math.log(0.05)):
    """Training set in the unit cube with a per-point noise a; theta = [log C, log l.., log w].  w itself comes from libm's
    exp, as the library's does, so that a + w formed here is the sum the device forms."""
    rng = np.random.default_rng(seed)
    X_ = rng.uniform(0, 1, (N, d))
    y_ = np.sin(3 * X_.sum(1)) + 0.2 * rng.standard_normal(N)
    a = rng.uniform(1e-4, 1e-2, N)
    theta = np.append(np.log(np.append(1.7, rng.uniform(0.2, 0.6, d))), log_w)
    return X_, y_, a, theta, math.exp(log_w)


# ------------------------------------------------------------------ 1 + 3: the shifted-alpha model, the white gradient entry
SHAPES = {"n33_d3": (33, 3, 0, 0), "n128_d16": (128, 16, 3, 0), "n129_d3": (129, 3, 2, 0), "n200_d17": (200, 17, 0, 0),
          "n2305_d4_tp": (2305, 4, 3, 1)}
_cache = {}


def shifted(dev, name):
    """(white model's results, plain model's with alpha = a + w), each evaluated once per shape."""
    if name in _cache:
        return _cache[name]
    N, d, kid, schedule = SHAPES[name]
    X_, y_, a, theta, w = problem(N, d, seed=N + d)
    Xq = np.random.default_rng(1).uniform(0, 1, (37, d))
    out = []
    dev.set_option("lml_schedule", schedule)
    try:
        for white in (True, False):
            dev.set_train(X_, y_, a if white else a + w)
            dev.set_theta(kid | W if white else kid, theta if white else theta[:-1])
            dev.set_affine()
            th = theta if white else theta[:-1]
            th2 = th.copy()                        # the objective away from the prediction factor's theta, at the same w
            th2[:d + 1] += 0.1
            if schedule:                           # the throughput schedule is a schedule of the batched call
                lml, grad, info = (v[0] for v in dev.lml_batch(th2[None, :], True))
                single = dev.lml(th2, True)        # ... and the latency chain at the same size
            else:
                lml, grad, info = dev.lml(th2, True)
                single = (lml, grad, info)
            assert info == 0 and single[2] == 0
            assert dev.factorize() == 0
            L, V, al = dev.get_factor()
            mean, std = dev.predict(Xq, return_std=True)
            out.append(dict(lml=lml, grad=grad, single=single, L=L, V=V, alpha_=al, mean=mean, std=std,
                            mean_only=dev.predict(Xq), mean_small=dev.predict(Xq[:3])))
    finally:
        dev.set_option("lml_schedule", 0)
    _cache[name] = (out[0], out[1], theta, w, d)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_model_a_w_is_todays_model_with_alpha_a_plus_w_to_the_bit(dev, name):
    wh, pl, theta, w, d = shifted(dev, name)
    for k in ("L", "V", "alpha_", "mean", "mean_only", "mean_small"):
        assert np.array_equal(wh[k], pl[k]), k
    assert wh["lml"] == pl["lml"] and wh["single"][0] == pl["single"][0]
    assert wh["grad"].shape == (d + 2,) and pl["grad"].shape == (d + 1,)
    assert np.array_equal(wh["grad"][:d + 1], pl["grad"]) and np.array_equal(wh["single"][1][:d + 1], pl["single"][1])
    # the white variance is in the predictive std: std_white^2 - std_plain^2 = w within 4 ulp of C + w
    prior = math.exp(theta[0]) + w
    assert np.max(np.abs((wh["std"] ** 2 - pl["std"] ** 2) - w)) <= 4 * np.spacing(prior)


@pytest.mark.parametrize("name", ["n129_d3", "n200_d17", "n2305_d4_tp"])
def test_white_gradient_entry_on_the_chain(dev, name):
    """1/2 w (|alpha_|^2 - |V|_F^2) in numpy from a factor at the objective's theta (which the test above pins to the
    existing arithmetic), on the paths the goldens do not reach."""
    N, d, kid, schedule = SHAPES[name]
    wh, pl, theta, w, _ = shifted(dev, name)
    X_, y_, a, _, _ = problem(N, d, seed=N + d)
    th2 = theta.copy()
    th2[:d + 1] += 0.1
    dev.set_train(X_, y_, a)
    dev.set_theta(kid | W, th2)
    assert dev.factorize() == 0
    _, V, al = dev.get_factor(want_L=False)
    ref = np.append(pl["grad"], wm.white_grad_from_factor(V, al, w))
    assert abs(ref[-1]) > 1e-3 * np.max(np.abs(ref))          # the entry is not hidden behind the others
    assert relmax(wh["grad"], ref) < 1e-7
    assert relmax(wh["single"][1], np.append(pl["single"][1], ref[-1])) < 1e-7


# ------------------------------------------------------------------ 2: against the reference
def load_golden_model(dev, g, p, kid):
    b = g[p + "bounds"]
    dev.set_train(g[p + "X_"], g[p + "y_"], g[p + "alpha"])
    dev.set_theta(kid | W, g[p + "theta"])
    dev.set_affine(b[:, 0], b[:, 1] - b[:, 0], float(g[p + "y_mean"]), float(g[p + "y_std"]))


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
def test_against_the_reference(dev, g, kid, s):
    p = f"k{kid}_s{s}_"
    theta, y_std = g[p + "theta"], float(g[p + "y_std"])
    load_golden_model(dev, g, p, kid)
    K = dev.kernel_train(add_alpha=False)              # kernel_(X_): w on the diagonal without alpha
    if s == 0:
        np.testing.assert_allclose(K, g[p + "K"], rtol=1e-13, atol=0)
    else:
        np.testing.assert_allclose(K[:16], g[p + "K_rows"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(np.diag(K), g[p + "K_diag"], rtol=1e-13, atol=0)
    Ka = dev.kernel_train(add_alpha=True)
    np.testing.assert_allclose(np.diag(Ka), np.diag(K) + g[p + "alpha"], rtol=1e-15)
    Xc = g[p + "Xc"]
    b = g[p + "bounds"]
    np.testing.assert_allclose(dev.kernel_cross((Xc - b[:, 0]) / (b[:, 1] - b[:, 0])), g[p + "Kx"], rtol=1e-13, atol=1e-300)
    lml, grad, info = dev.lml(theta, True)
    assert info == 0 and grad.shape == g[p + "grad"].shape
    assert abs(lml - g[p + "lml"]) <= 1e-10 * abs(g[p + "lml"])
    assert relmax(grad, g[p + "grad"]) < 1e-7
    assert dev.lml(theta, False)[0] == lml
    assert dev.factorize() == 0
    mean, std = dev.predict(Xc, return_std=True)
    np.testing.assert_allclose(mean, g[p + "mean"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(std, g[p + "std"], rtol=1e-6, atol=1e-9)
    prior = (math.exp(theta[0]) + math.exp(theta[-1])) * y_std ** 2
    assert np.max(np.abs(std ** 2 - g[p + "std"] ** 2)) <= 1e-9 * prior
    np.testing.assert_allclose(dev.predict(Xc), mean, rtol=1e-9, atol=1e-10)
    # LogExp through the sweep: the reference subtracts the FIXED noise level, not w
    out = dev.sweep_logexp(Xc, float(g[p + "zeta"]), float(np.max(g[p + "y"])), float(np.mean(g[p + "noise_level"])))
    assert out["n_nan"] == 0
    np.testing.assert_allclose(out["acq"], g[p + "acq"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out["sigma"], g[p + "std"], rtol=1e-6, atol=1e-9)
    if s == 0:
        # the kernel object itself, through the scratch context: kernel_(X) has w on its diagonal, kernel_(X, Y) has none
        from gpry_amd.kernels import RBF, ConstantKernel as Ck, Matern, WhiteKernel
        stat = RBF([1.0] * 2, [1e-3, 10.]) if kid == 0 else Matern([1.0] * 2, [1e-3, 10.], nu={1: 0.5, 2: 1.5, 3: 2.5}[kid])
        kern = Ck(1.0, [1e-4, 1e6]) * stat + WhiteKernel(1.0, [1e-6, 1e2])
        kern.theta = theta
        Xc_ = (Xc - b[:, 0]) / (b[:, 1] - b[:, 0])
        np.testing.assert_allclose(kern(g[p + "X_"]), g[p + "K"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(kern(Xc_, g[p + "X_"]), g[p + "Kx"], rtol=1e-13, atol=1e-300)
        np.testing.assert_array_equal(kern.gradient_x(Xc_[0], g[p + "X_"]), kern.k1.gradient_x(Xc_[0], g[p + "X_"]))
        load_golden_model(dev, g, p, kid)                  # (the scratch context is another context: nothing to restore,
        assert dev.factorize() == 0                        # but the next lines read `dev` as this test left it)
    if kid == 1:
        return                                             # (the reference's own x-gradient of Matern-1/2 raises)
    mb, sb, mgb, kgb = dev.predict_grad_batch(Xc)
    for i, x in enumerate(Xc):
        m1, s1, mg, kg, _ = dev.predict_point(x)
        for mean1, std1, mgrad, kgrad in ((m1, s1, mg, kg), (mb[i], sb[i], mgb[i], kgb[i])):
            assert mean1 == pytest.approx(g[p + "mean"][i], rel=1e-8, abs=1e-9)
            assert std1 == pytest.approx(g[p + "std"][i], rel=1e-6, abs=1e-9)
            np.testing.assert_allclose(mgrad * y_std, g[p + "mean_grad"][i], rtol=1e-7,
                                       atol=1e-8 * np.max(np.abs(g[p + "mean_grad"])))
            np.testing.assert_allclose(-kgrad / (std1 / y_std) * y_std * y_std, g[p + "std_grad"][i], rtol=1e-6,
                                       atol=1e-8 * np.max(np.abs(g[p + "std_grad"])))


# ------------------------------------------------------------------ 4: gpry_lml_batch
@pytest.mark.parametrize("N", [200, 64])
def test_lml_batch_every_theta_its_own_w(dev, N):
    d, kid = 3, 2
    X_, y_, _, theta, _ = problem(N, d, seed=5)
    X_[N // 2] = X_[3]
    X_[N - 1] = X_[7]                                  # duplicate rows: w alone keeps the matrix positive definite
    dev.set_train(X_, y_, np.zeros(N))
    dev.set_theta(kid | W, theta)
    thetas = np.array([theta,
                       np.append(theta[:-1], math.log(0.3)),                 # differs in w alone
                       theta + np.array([0.4, -0.3, 0.2, 0.1, -1.0]),        # differs in everything
                       np.append(theta[:-1], -40.0)])                        # not positive definite
    singles = [dev.lml(th, True) for th in thetas]
    lml, grad, info = dev.lml_batch(thetas, True)
    for b, (l1, g1, i1) in enumerate(singles):
        assert lml[b] == l1 and np.array_equal(grad[b], g1) and info[b] == i1, b
    assert np.isneginf(lml[3]) and not grad[3].any() and info[3] > 0
    assert np.isfinite(lml[:3]).all() and not info[:3].any() and len({float(v) for v in lml[:3]}) == 3
    assert grad[0][-1] != grad[1][-1] and np.array_equal(lml, dev.lml_batch(thetas, False)[0])
    bad = dev.lml_batch(thetas[3:], True)
    assert np.isneginf(bad[0][0]) and not bad[1].any() and bad[2][0] > 0
    # ... and against the closed form
    for b in range(3):
        ref = wm.lml(X_, y_, np.zeros(N), thetas[b], kid, eval_gradient=True)
        assert abs(lml[b] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(grad[b], ref[1]) < 1e-7


# ------------------------------------------------------------------ 5: append_rows, loo
def test_append_rows_borders_with_the_white_term(dev):
    N0, k, d, kid = 126, 4, 3, 3
    X_, y_, a, theta, w = problem(N0 + k, d, seed=11)
    fresh = _device()
    try:
        fresh.set_train(X_, y_, a)
        fresh.set_theta(kid | W, theta)
        fresh.set_affine(y_mean=0.3, y_std=1.7)
        assert fresh.factorize() == 0
        L0, V0, a0 = fresh.get_factor()
        dev.set_train(X_[:N0], y_[:N0], a[:N0])
        dev.set_theta(kid | W, theta)
        dev.set_affine(y_mean=0.3, y_std=1.7)
        assert dev.factorize() == 0
        assert dev.append_rows(X_[N0:], y_[N0:], a[N0:]) == 0 and dev.N == N0 + k
        L1, V1, a1 = dev.get_factor()
        np.testing.assert_allclose(L1, L0, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(V1, V0, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(a1, a0, rtol=1e-8, atol=1e-9)
        Xq = np.random.default_rng(2).uniform(0, 1, (33, d))
        for u, v in zip(dev.predict(Xq, return_std=True), fresh.predict(Xq, return_std=True)):
            np.testing.assert_allclose(u, v, rtol=1e-8, atol=1e-9)
        for res in (dev.loo(), fresh.loo()):
            # the latent variance leaves out the point's whole noise, a_i + w; var_y is untouched
            np.testing.assert_allclose(res["var_f"], np.maximum(res["var_y"] - (a + w) * 1.7 ** 2, 0.0), rtol=1e-12, atol=1e-15)
            assert (res["var_f"] > 0).any()
        m = wm.WhiteModel(X_, y_, a, kid, theta, y_mean=0.3, y_std=1.7)
        Kinv = m.V.T @ m.V
        np.testing.assert_allclose(dev.loo()["var_y"], 1.7 ** 2 / np.diag(Kinv), rtol=1e-8)
    finally:
        fresh.close()


# ------------------------------------------------------------------ 6: sweep, pruned sweep, Kriging believer
SWEEP_N, SWEEP_D, SWEEP_M, SWEEP_KID = 200, 4, 20_000, 3


def sweep_problem(short=False):
    """w = 0.05 C.  ``short``: one length scale far below the extent of the data (the hybrid panel form), the candidates
    aligned with training rows in that coordinate so that they still see the data.  Seed 79: in the closed form the 64th
    and 65th acquisition values of the pool differ by 2.8e-3 (ordinary model) and 2.5e-3 (short), checked on the CPU."""
    rng = np.random.default_rng(79)
    N, d = SWEEP_N, SWEEP_D
    bounds = np.array([[-2.0, 3.0]] * d)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (N, d))
    y = -0.5 * ((X - 0.5) ** 2).sum(1) + 0.3 * rng.standard_normal(N)
    Xc = rng.uniform(bounds[:, 0], bounds[:, 1], (SWEEP_M, d))
    Xc[:50] = X[:50] + 1e-3 * rng.standard_normal((50, d))            # candidates next to training points
    C = 2.0
    ls = [1e-4, 0.3, 0.25, 0.35] if short else [0.3, 0.25, 0.35, 0.3]
    if short:
        Xc[:, 0] = X[rng.integers(N, size=SWEEP_M), 0]
    theta = np.log(np.array([C] + ls + [0.05 * C]))
    return bounds, X, y, Xc, theta


def sweep_gpr(short=False):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, Matern, WhiteKernel, clone
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    bounds, X, y, Xc, theta = sweep_problem(short)
    kernel = Ck(1.0, [1e-4, 1e6]) * Matern([1.0] * SWEEP_D, [1e-5, 10.], nu=2.5) + WhiteKernel(1.0, [1e-6, 1e2])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=bounds, noise_level=1e-2, optimizer=None,
                                   preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(), account_for_inf=None)
    k = clone(kernel)
    k.theta = theta
    gpr.kernel_, gpr._fitted = k, True
    gpr.append_to_data(X, y, fit_gpr=False)
    gpr._ensure_factor()
    gpr._push_affine()
    return bounds, Xc, theta, gpr


def closed_form(gpr, theta, bounds):
    lo, span, y_mean, y_std, clip_hi = gpr._affine_args()         # (the mean is clipped at clip_factor * y_max)
    np.testing.assert_array_equal(lo, bounds[:, 0])
    return wm.WhiteModel(gpr.X_train_, gpr.y_train_, gpr.alpha, SWEEP_KID, theta, lo, span, y_mean, y_std, clip_hi)


def test_sweep_in_all_panel_forms_and_the_pruned_shortlist():
    zeta = orc.auto_zeta(SWEEP_D)
    for short, options, form in ((False, {}, "mfma"), (False, {"cross_mfma": 0}, "difference"), (True, {}, "hybrid")):
        bounds, Xc, theta, gpr = sweep_gpr(short)
        dev = gpr.device
        m = closed_form(gpr, theta, bounds)
        rm, rs = m.predict(Xc)
        racq = m.logexp(Xc, zeta, gpr.y_max, gpr.noise_level)
        order = np.argsort(-racq, kind="stable")
        assert racq[order[63]] - racq[order[64]] > 1e-6           # exact equality below tests the bound, not a tie
        for k, v in options.items():
            dev.set_option(k, v)
        out = dev.sweep_logexp(Xc, zeta, gpr.y_max, gpr.noise_level)
        assert dev.sweep_info()["panel_form"] == form and out["n_nan"] == 0
        prior = (m.C + m.w) * m.y_std ** 2
        np.testing.assert_allclose(out["y"], rm, rtol=1e-8, atol=1e-8)
        assert np.max(np.abs(out["sigma"] ** 2 - rs ** 2)) <= 1e-9 * prior
        fin = np.isfinite(racq)
        np.testing.assert_allclose(out["acq"][fin], racq[fin], rtol=1e-6, atol=1e-6)
        # with a fitted w the acquisition does not fall to -inf next to training points (the reference's behaviour)
        assert np.isfinite(out["acq"][:50]).all() and (out["sigma"][:50] ** 2 > 0.9 * m.w * m.y_std ** 2).all()
        # given y, and given y and sigma: the same finish
        giv = dev.sweep_logexp(Xc, zeta, gpr.y_max, gpr.noise_level, y_given=out["y"])
        assert np.array_equal(giv["sigma"], out["sigma"]) and np.array_equal(giv["acq"], out["acq"])
        giv = dev.sweep_logexp(Xc, zeta, gpr.y_max, gpr.noise_level, y_given=out["y"], sigma_given=out["sigma"])
        assert np.array_equal(giv["acq"], out["acq"])
        # the pruned sweep: its sigma bound is the prior sigma sqrt(C + w); the shortlist is the full sweep's, exactly
        dev.sweep_logexp(Xc, zeta, gpr.y_max, gpr.noise_level, want=())
        full, fb = dev.sweep_topk(64)
        dev.set_option("sweep_prune", 1)
        try:
            dev.sweep_logexp(None, zeta, gpr.y_max, gpr.noise_level, M=len(Xc), want=())
        finally:
            dev.set_option("sweep_prune", 0)
        pruned, pb = dev.sweep_topk(64)
        assert dev.sweep_prune_info()["M"] == len(Xc)
        for f in ("idx", "acq", "y", "sigma"):
            assert np.array_equal(pruned[f], full[f]), (form, f)
        assert pb >= fb and np.array_equal(full["idx"], order[:64])
        got = dev.sweep_fetch(("y", "sigma", "acq"))
        for k in ("y", "sigma", "acq"):
            assert np.array_equal(got[k], out[k]), (form, k)


def test_multi_add_and_kriging_believer_variances():
    from gpry_amd.gp_acquisition import NORA
    res = {}
    for prune in (True, False):
        bounds, Xc, theta, gpr = sweep_gpr()
        acq = NORA(bounds, sampler="uniform", mc_every=2, verbose=0, exact_prune=prune)
        acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
        res[prune] = acq.multi_add(gpr, n_points=4, rng=np.random.default_rng(2))
        assert (acq.stats.get("prune") is not None) == prune
    for u, v in zip(res[True], res[False]):
        assert np.array_equal(u, v)
    Xp = res[True][0]
    assert Xp.shape == (4, SWEEP_D)
    # var0 of a session and the conditioned std against the closed form with the lies appended at alpha + w
    bounds, Xc, theta, gpr = sweep_gpr()
    m = closed_form(gpr, theta, bounds)
    s = gpr.kb_session()
    idx = s.register(Xc[:300])
    np.testing.assert_allclose(s.var0[idx], m.var0(Xc[:300]), rtol=0, atol=1e-9 * (m.C + m.w))
    assert s.noise_alpha() == float(np.ravel(gpr.alpha)[0]) + m.w
    lies = Xc[300:303]
    cond = gpr.conditioned(lies, gpr.predict(lies))
    m2 = wm.WhiteModel(np.vstack([gpr.X_train_, m.unit(lies)]), np.append(gpr.y_train_, np.zeros(3)),
                       np.append(np.broadcast_to(gpr.alpha, (SWEEP_N,)), np.full(3, np.ravel(gpr.alpha)[0])), SWEEP_KID, theta,
                       bounds[:, 0], bounds[:, 1] - bounds[:, 0], gpr.preprocessing_y.mean_, gpr.preprocessing_y.std_)
    got = cond.predict_std(Xc[:300])
    assert np.max(np.abs(got ** 2 - m2.predict(Xc[:300])[1] ** 2)) <= 1e-9 * (m.C + m.w) * m.y_std ** 2


# ------------------------------------------------------------------ 7: the fit
@pytest.mark.parametrize("lockstep", [True, False])
def test_fit_learns_the_noise_level(g, lockstep):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    bounds, X, y = g["fit_bounds"], g["fit_X"], g["fit_y"]
    kernel = Ck(1.0, [1e-3, 1e4]) * RBF([1.0, 1.0], [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=bounds, n_restarts_optimizer=int(g["fit_n_restarts"]), noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=3)
    gpr.fit_lockstep = lockstep
    gpr.append_to_data(X, y, fit_gpr=True)
    assert gpr.fit_stats["side_by_side"] == lockstep
    lml_ref = float(g["fit_lml"])
    print(f"fit (side by side: {lockstep}): lml {gpr.log_marginal_likelihood_value_:.9f} (reference {lml_ref:.9f}), theta {gpr.kernel_.theta}")
    # the device's optimum may be another one, never a worse one
    assert gpr.log_marginal_likelihood_value_ >= lml_ref - 1e-6 * abs(lml_ref)
    # the reference's fitted theta evaluated here gives the reference's LML
    assert abs(gpr.log_marginal_likelihood(g["fit_theta"]) - lml_ref) <= 1e-10 * abs(lml_ref)
    w, target = float(np.exp(gpr.kernel_.theta[-1])), 0.09 / float(g["fit_y_std"]) ** 2
    assert target / 2 < w < 2 * target
    # the fitted model predicts with its noise: std^2 >= w y_std^2 everywhere
    std = gpr.predict(X[:20], return_std=True)[1]
    assert (std ** 2 >= 0.999 * w * float(g["fit_y_std"]) ** 2).all()


# ------------------------------------------------------------------ 8: everything else
def test_mean_only_consumers_and_the_resident_server():
    from gpry_amd.maximize import hessian_gp, maximize_gp
    from gpry_amd.mc import mc_sample_from_gp
    bounds, Xc, theta, gpr = sweep_gpr()
    m = closed_form(gpr, theta, bounds)
    dev = gpr.device
    # one point through the resident kernel = the batched predict
    batched = dev.predict(Xc[:64])
    requests0 = dev.serve_stats()[1]
    one = np.array([dev.predict(Xc[i:i + 1])[0] for i in range(8)])
    assert dev.serve_stats()[1] >= requests0 + 8
    np.testing.assert_allclose(one, batched[:8], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(batched, m.predict(Xc[:64])[0], rtol=1e-8, atol=1e-9)
    Xs, ys, ws = mc_sample_from_gp(gpr, sampler="mcmc", seed=3, sampler_options={"max_samples": 4000})
    assert len(Xs) > 50 and np.isfinite(ys).all()
    np.testing.assert_allclose(ys[:200], m.predict(Xs[:200])[0], rtol=1e-8, atol=1e-9)
    res = maximize_gp(gpr, nstarts=8)
    np.testing.assert_allclose(res.y_all, m.predict(res.X_all)[0], rtol=1e-8, atol=1e-9)
    yh, gh, Hh = hessian_gp(gpr, res.X_all[:3])
    np.testing.assert_allclose(yh, m.predict(res.X_all[:3])[0], rtol=1e-8, atol=1e-9)
    assert np.isfinite(Hh).all() and np.array_equal(Hh, np.swapaxes(Hh, 1, 2))


def test_refusals_name_the_white_term_and_leave_the_context_intact():
    from gpry_amd import _lib
    from gpry_amd.gp_acquisition import BatchOptimizer
    bounds, Xc, theta, gpr = sweep_gpr()
    dev = gpr.device
    before = dev.predict(Xc[:40], return_std=True)
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    calls = {
        "gpry_maximize_acq": lambda: dev.maximize_acq(lo, hi, Xc[:4], np.zeros(SWEEP_D, bool), np.eye(SWEEP_D), 1.0,
                                                      0.0, 0.01, 10, 4, 1e-6, 0.0, -np.inf),
        "gpry_predict_cov": lambda: dev.predict_cov(Xc[:8]),
        "gpry_sample_joint": lambda: dev.sample_joint(Xc[:8], 4, 1),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.GpryHipError, match="white term") as e:
            call()
        assert name in str(e.value)
        after = dev.predict(Xc[:40], return_std=True)           # the next call is answered, and answered as before
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    with pytest.raises(NotImplementedError, match="white term"):
        gpr.predict(Xc[:8], return_cov=True)
    with pytest.raises(NotImplementedError, match="white term"):
        gpr.sample_y(Xc[:8], 2)
    with pytest.raises(NotImplementedError, match="white term"):
        # (the group's Python side refuses before anything reaches a member; the library's own refusal needs a group)
        _lib.DeviceGroup.set_model(object.__new__(_lib.DeviceGroup), gpr.X_train_, gpr.y_train_, gpr.alpha, *gpr._device_theta())
    # the device optimiser of the acquisition falls back to the side-by-side L-BFGS-B runs
    opt = BatchOptimizer(bounds, preprocessing_X=gpr.preprocessing_X, acq_optimizer="device", n_restarts_optimizer=4, verbose=0)
    Xp, yp, ap = opt.multi_add(gpr, n_points=1, rng=np.random.default_rng(1))
    assert Xp.shape == (1, SWEEP_D) and np.isfinite(ap).all()
    after = gpr.device.predict(Xc[:40], return_std=True)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


def test_a_plain_model_after_a_white_one_keeps_its_bits(dev):
    N, d, kid = 150, 3, 2
    X_, y_, a, theta, w = problem(N, d, seed=21)
    Xq = np.random.default_rng(3).uniform(0, 1, (300, d))

    def plain():
        dev.set_train(X_, y_, a)
        dev.set_theta(kid, theta[:-1])
        dev.set_affine()
        lml = dev.lml(theta[:-1] + 0.1, True)
        lb = dev.lml_batch(np.array([theta[:-1], theta[:-1] - 0.2]), True)
        assert dev.factorize() == 0
        sw = dev.sweep_logexp(Xq, 1.0, 0.0, 0.01)
        return (lml[0], lml[1], lb[0], lb[1], *dev.get_factor(), *dev.predict(Xq, return_std=True), dev.predict(Xq[:2]),
                dev.kernel_train(True), sw["y"], sw["sigma"], sw["acq"], dev.loo()["var_f"], dev.kb_register(Xq[:5])[1])

    first = plain()
    dev.set_theta(kid | W, theta)
    assert dev.factorize() == 0 and dev.lml(theta, True)[1].shape == (d + 2,)
    dev.lml_batch(np.array([theta, theta + 0.1]), True)
    dev.sweep_logexp(Xq, 1.0, 0.0, 0.01)
    assert dev.predict(Xq, return_std=True)[1].min() ** 2 >= w * 0.999
    second = plain()
    assert first[1].shape == (d + 1,)
    for u, v in zip(first, second):
        assert np.array_equal(u, v)
