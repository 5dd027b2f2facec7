"""Hessian of the surrogate's mean on the device (gpry_amd/csrc/hessian.hip + gpry_amd/maximize.py: hessian_gp,
laplace_gp, covmat="laplace"): H and g against the closed form of tests/tools/hessian_numpy.py at every (tile shape,
kernel id, slice shape), y the one-point predict's bits, H symmetric to the last bit; a point's bits depend on the model
and the point alone; a gated point keeps its derivatives; Matern 1/2 and ill-formed arguments are refused with a message;
laplace_gp and maximize_gp(covmat="laplace") agree with the host route on the oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_mcmc_gpu import _pushed
from test_nested_gpu import _one_point, _svm_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hessian_numpy as hn  # noqa: E402
import maximize_numpy as mn  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- against the stand-in ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [100, 1100, 2500])
@pytest.mark.parametrize("d", [2, 5, 9, 16, 17, 32])
@pytest.mark.parametrize("kid", [sw.RBF, sw.M32, sw.M52])
def test_hessian_gradient_and_value_against_the_stand_in(kid, d, N):
    """8 training rows and 16 random points: H and g within 1e-7 of the largest entry of each (the tolerance the
    gradient of the ascents is held to), y bit for bit the one-point predict's, H == H.T exactly."""
    affine = (kid + d + N // 1000) % 2 == 0
    model = sw.Model(d, kid, N, affine=affine, seed=N + d)
    gpr = _pushed(model.gpr())
    deriv = hn.MeanDerivatives.of_oracle(model.oracle(gpr))
    lo, hi = np.full(d, -3.0), np.full(d, 3.5)
    rng = np.random.default_rng(kid + 10 * d)
    X = np.ascontiguousarray(np.concatenate([gpr.X_train[rng.choice(N, 8, replace=False)], rng.uniform(lo, hi, (16, d))]))
    out = gpr.device.hessian_mean(X)
    g, H = deriv.grad_hess(X)
    eg, eh = _rel(out["g"], g), _rel(out["H"], H)
    rows = max(_rel(out["H"][i], H[i]) for i in range(8))
    print(f"kid={kid} d={d} N={N} affine={affine}: |H - ref| / max|ref| = {eh:.3e} (per point at training rows "
          f"{rows:.3e}), |g - ref| / max|ref| = {eg:.3e}, device {out['device_ms']:.3f} ms")
    assert np.max(np.abs(H)) > 0 and np.max(np.abs(g)) > 0
    assert eh <= 1e-7 and eg <= 1e-7
    for i in range(len(X)):
        assert _rel(out["H"][i], H[i]) <= 1e-7, i
    np.testing.assert_array_equal(out["y"], _one_point(gpr, X))
    np.testing.assert_array_equal(out["H"], np.swapaxes(out["H"], 1, 2))


# ---- independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margs", [dict(d=4, kid=sw.M52, N=1500), dict(d=17, kid=sw.RBF, N=2500),
                                   dict(d=32, kid=sw.M32, N=300)], ids=lambda m: f"d={m['d']} N={m['N']}")
def test_same_bits_alone_in_a_batch_at_any_position_in_split_calls_and_on_a_second_context(margs):
    model = sw.Model(seed=2, **margs)
    gpr, gpr2 = _pushed(model.gpr()), _pushed(model.gpr())
    assert gpr2.device is not gpr.device
    d, n = model.d, 1000
    rng = np.random.default_rng(3)
    X = rng.uniform(-3.0, 3.0, (n, d))
    X[:50] = gpr.X_train[rng.choice(len(gpr.X_train), 50, replace=False)]
    a, b = gpr.device.hessian_mean(X), gpr2.device.hessian_mean(X)
    h1, h2 = gpr.device.hessian_mean(X[:300]), gpr.device.hessian_mean(X[300:])
    perm = rng.permutation(n)
    p = gpr.device.hessian_mean(np.ascontiguousarray(X[perm]))
    for key in ("y", "g", "H"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a[key], np.concatenate([h1[key], h2[key]]), err_msg=key)
        np.testing.assert_array_equal(a[key][perm], p[key], err_msg=key)
        for i in (0, 49, 777, n - 1):
            np.testing.assert_array_equal(gpr.device.hessian_mean(X[i:i + 1])[key][0], a[key][i], err_msg=f"{key} {i}")
    assert np.all(np.isfinite(a["H"])) and np.all(np.isfinite(a["g"]))


# ---- gates ------------------------------------------------------------------------------------------------------------
def test_a_gated_point_has_y_minus_inf_and_the_derivatives_of_the_ungated_model():
    gpr, bounds = _svm_model()
    _pushed(gpr)
    rng = np.random.default_rng(1)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (64, 3))
    X[:8, 0] = rng.uniform(2.0, 3.9, 8)                     # the classifier's rejected side
    on = gpr.device.hessian_mean(X)
    gated = np.isneginf(on["y"])
    assert gated[:8].all() and 8 <= gated.sum() < 64
    np.testing.assert_array_equal(on["y"], _one_point(gpr, X))
    gpr.device.set_gates()
    off = gpr.device.hessian_mean(X)
    assert np.all(np.isfinite(off["y"]))
    np.testing.assert_array_equal(on["H"], off["H"])
    np.testing.assert_array_equal(on["g"], off["g"])
    np.testing.assert_array_equal(on["y"][~gated], off["y"][~gated])
    assert np.all(np.isfinite(on["H"])) and np.all(np.isfinite(on["g"]))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_matern12_is_refused_by_the_call_and_by_hessian_gp():
    from gpry_amd._lib import GpryHipError
    from gpry_amd.mc import hessian_gp, laplace_gp, maximize_gp
    gpr = _pushed(sw.Model(3, sw.M12, 200).gpr())
    X = np.zeros((2, 3))
    y, g, H = np.empty(2), np.empty((2, 3)), np.empty((2, 3, 3))
    dev = gpr.device
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    assert dev._lib.gpry_hessian_mean(dev._h, vp(X), 2, vp(y), vp(g), vp(H), None) == -1
    msg = dev._lib.gpry_last_error(dev._h).decode()
    assert "Matern-1/2" in msg and "not differentiable" in msg
    with pytest.raises(GpryHipError, match="Matern-1/2"):
        dev.hessian_mean(X)
    for call in (lambda: hessian_gp(gpr, X), lambda: laplace_gp(gpr), lambda: maximize_gp(gpr, covmat="laplace")):
        with pytest.raises(ValueError, match="Matern-1/2"):
            call()


def test_bad_arguments_are_refused_with_a_message():
    from gpry_amd._lib import Device, GpryHipError
    gpr = _pushed(sw.Model(3, sw.M52, 200).gpr())
    dev = gpr.device
    X = np.zeros((2, 3))
    y, g, H = np.empty(2), np.empty((2, 3)), np.empty((2, 3, 3))
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731

    def call(X=X, n=2, y=y, g=g, H=H):
        rc = dev._lib.gpry_hessian_mean(dev._h, vp(X), n, vp(y), vp(g), vp(H), None)
        return rc, dev._lib.gpry_last_error(dev._h).decode()

    assert call()[0] == 0
    for kw, word in ((dict(n=0), "npts"), (dict(n=-3), "npts"), (dict(n=2**31), "npts"), (dict(H=None), "NULL"),
                     (dict(X=None), "NULL"), (dict(y=None), "NULL"), (dict(g=None), "NULL"),
                     (dict(X=np.array([[0.0, np.nan, 0.0], [0.0] * 3])), "not finite"),
                     (dict(X=np.array([[0.0] * 3, [np.inf, 0.0, 0.0]])), "not finite")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and "gpry_hessian_mean" in msg, (kw, rc, msg)
    with pytest.raises(GpryHipError, match="not finite"):
        dev.hessian_mean(np.full((1, 3), np.nan))
    with pytest.raises(ValueError):
        dev.hessian_mean(np.zeros((2, 4)))
    # no model
    fresh = Device(dev.device)
    fresh.d = 3
    with pytest.raises(GpryHipError, match="gpry_hessian_mean|model|train"):
        fresh.hessian_mean(X)
    fresh.close()


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mn.E2E_MODELS))
def test_laplace_gp_and_the_laplace_h0_agree_with_the_host_route_on_the_oracle(name):
    from gpry_amd.mc import hessian_gp, laplace_gp, maximize_gp
    m = sw.Model(**mn.E2E_MODELS[name])
    ogpr, deriv = hn.oracle_gpr(m)
    gpr = m.gpr()
    before = gpr.n_eval
    r0 = maximize_gp(gpr, nstarts=32)
    r = laplace_gp(gpr, nstarts=32)
    assert gpr.n_eval - before == 2 * int(r0.ncalls.sum()) + 1
    np.testing.assert_array_equal(r.x, r0.x)
    assert r.y == r0.y
    H = deriv.grad_hess(r.x[None])[1][0]
    k = int(r.free.sum())
    err = _rel(r.H, H)
    inv = float(np.max(np.abs(r.cov @ (-r.H[np.ix_(r.free, r.free)]) - np.eye(k))))
    ref = laplace_gp(ogpr, nstarts=32)
    print(f"{name}: |H - ref| / max|ref| = {err:.3e}; |cov (-H_ff) - I| = {inv:.3e}; logZ {r.logZ:.9g} (oracle "
          f"{ref.logZ:.9g}); device {1e3 * r.device_s:.2f} ms")
    assert err <= 1e-7
    assert inv <= 1e-8
    np.testing.assert_array_equal(r.free, ref.free)
    assert r.negdef == ref.negdef and r.negdef and r.free.all()
    y, g, Hb = hessian_gp(gpr, np.stack([r.x, r.x]))
    np.testing.assert_array_equal(Hb[0], r.H)
    np.testing.assert_array_equal(Hb[1], r.H)
    # the Laplace H0 ends at the same maxima as the default
    rl = maximize_gp(gpr, nstarts=32, covmat="laplace")
    tol = 2 * m.tol()
    print(f"{name}: best y {rl.y:.12g} with the Laplace H0, {r0.y:.12g} with the default (tolerance {tol:.3e}); iterations "
          f"{int(rl.iters.sum())} against {int(r0.iters.sum())}; distinct maxima {rl.n_distinct} and {r0.n_distinct}")
    assert rl.n_distinct == r0.n_distinct
    assert abs(rl.y - r0.y) <= tol
