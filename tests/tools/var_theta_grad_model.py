"""numpy float64 closed form of the derivative of a GP's latent predictive variance in theta, the reference of the
``gpry_var_theta_grad`` tests, the assertions both test files share and a stand-in device.

theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last; K = C phi(r) + diag(alpha [+ w]), k the
cross-kernel row of a point, dk_a = d k / d log l_a = C h(r) diff_a^2 (``theta_grad_model.cross_terms``), dK_a = dK / dlog l_a
among the training rows, q = K^-1 k and var = y_std^2 (C + w - k^T q):
    G_0 = y_std^2 ((C - k^T q) - sum_i (alpha_i + w) q_i^2)
    G_a = y_std^2 (-2 q . dk_a + q^T dK_a q)
    G_w = y_std^2 w (1 + |q|^2)
Two formulations: (a) ``grad_explicit`` with the explicit symmetrised inverse and the explicit dK_a; (b) ``grad_via_V``
through V = L^-1 with q = V^T (V k) and k^T q = |V k|^2.  ``var_numpy`` is the refactorised variance
(``predict_thetas_var_model.var_numpy``), ``central_differences`` differentiates it.  Points are in the unit (transformed)
coordinates here; the checks map them through the x-affine.

The tolerance of a device against (b) is ``theta_grad_model.column_bound``, per column j of G:
    max|G_dev - G_b|_j <= max(10 max|G_a - G_b|_j, 1e-7 max|G_b|_j)

``VarThetaGradDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU; its three switches make the
broken variants the checks must catch.  Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from loo_fit_model import _matrices, problem  # noqa: F401
from theta_grad_model import (CASES, IDS, W_FLAG, Y_MEAN, Y_STD, ThetaGradDevice, affine, column_bound, column_dev,  # noqa: F401
                              cross_terms, load, points, to_raw)
from predict_thetas_var_model import PredictThetasVarDevice, prior_var, var_numpy, var_via_V  # noqa: F401


def _assemble(k, dk, q, kq, dKs, noise_w, theta, d, white, ys2, quad_sign=1.0, cross_factor=2.0, logc_noise=True):
    """(var (M,), G (M, p)) from the rows k, dk, q (M, N) and kq = k^T q per point."""
    C = math.exp(theta[0])
    w = math.exp(theta[d + 1]) if white else 0.0
    G = np.empty((k.shape[0], d + 1 + int(white)))
    G[:, 0] = (C - kq) - (np.einsum("mi,i,mi->m", q, noise_w, q) if logc_noise else 0.0)
    for a in range(d):
        G[:, 1 + a] = -cross_factor * np.einsum("mi,mi->m", q, dk[:, :, a]) + quad_sign * np.einsum("mi,ij,mj->m", q, dKs[1 + a], q)
    if white:
        G[:, d + 1] = w * (1.0 + np.einsum("mi,mi->m", q, q))
    return ys2 * ((C + w) - kq), ys2 * G


def _noise_w(alpha, theta, d, white, N):
    return np.broadcast_to(alpha, (N,)) + (math.exp(theta[d + 1]) if white else 0.0)


def grad_explicit(X_, alpha, theta, kid, white, Xq_, y_std=1.0):
    """Formulation (a): ``(var, G)`` with the explicit symmetrised inverse."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    k, dk = cross_terms(Xq_, X_, theta, kid)
    q = k.dot(Kinv)
    return _assemble(k, dk, q, np.einsum("mi,mi->m", k, q), dKs, _noise_w(alpha, theta, d, white, len(X_)), theta, d, white,
                     y_std * y_std)


def grad_via_V(X_, alpha, theta, kid, white, Xq_, y_std=1.0, **broken):
    """Formulation (b): ``(var, G)`` through V = L^-1, q = V^T (V k), k^T q = |V k|^2."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    V = solve_triangular(cholesky(K, lower=True), np.eye(len(X_)), lower=True)
    k, dk = cross_terms(Xq_, X_, theta, kid)
    t = k.dot(V.T)                                      # rows: (V k)^T
    q = t.dot(V)
    return _assemble(k, dk, q, np.einsum("mi,mi->m", t, t), dKs, _noise_w(alpha, theta, d, white, len(X_)), theta, d, white,
                     y_std * y_std, **broken)


def central_differences(X_, alpha, theta, kid, white, Xq_, y_std=1.0, h=1e-4):
    """Central differences of ``var_numpy`` in every entry of theta (truncation O(h^2))."""
    theta = np.asarray(theta, dtype=float)
    G = np.empty((len(Xq_), len(theta)))
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        G[:, j] = (var_numpy(X_, alpha, theta + e, kid, white, Xq_, y_std)
                   - var_numpy(X_, alpha, theta - e, kid, white, Xq_, y_std)) / (2.0 * h)
    return G


# ---------------------------------------------------------------------------------------------- the stand-in
class VarThetaGradDevice(PredictThetasVarDevice):
    """``ThetaGradDevice`` (through ``PredictThetasVarDevice``, whose ``predict_thetas`` the checks difference) with
    ``var_theta_grad``: formulation (b) at the factorised theta, one point at a time, so that -- as on the device -- a point's
    bits do not depend on the batch it comes in."""
    n_vtg = 0
    quad_sign = 1.0          # the broken variants of the CPU tests turn these
    cross_factor = 2.0
    logc_noise = True

    def var_theta_grad(self, X, want_var=True):
        self.n_vtg += 1
        assert self._factor is not None, "model not factorised"
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        assert len(X) >= 1 and np.all(np.isfinite(X))
        var, G = np.empty(len(X)), np.empty((len(X), self.n_theta))
        for i, x_ in enumerate(self._to_unit(X)):
            v, g = grad_via_V(self.X_, self.alpha, self.theta_full, self.kid, self.white, x_[None, :], self.y_std,
                              quad_sign=self.quad_sign, cross_factor=self.cross_factor, logc_noise=self.logc_noise)
            var[i], G[i] = v[0], g[0]
        return {"var": var if want_var else None, "G": G, "device_ms": 0.0}


assert issubclass(VarThetaGradDevice, ThetaGradDevice)


# ---------------------------------------------------------------------------------------------- the references
_ref = {}


def reference(case):
    """(Xq_ unit points, G_a, G_b, var_a, var_b) of the case, computed once and never changed: G of the two formulations
    here, var of ``predict_thetas_var_model``'s two (the triangular solve and the explicit V)."""
    if case not in _ref:
        N, d, kid, white = case
        X_, y_, a, th = problem(N, d, seed=N + d, white=white)
        Xq_ = points(case, X_)
        _, Ga = grad_explicit(X_, a, th, kid, white, Xq_, Y_STD)
        _, Gb = grad_via_V(X_, a, th, kid, white, Xq_, Y_STD)
        va, vb = var_numpy(X_, a, th, kid, white, Xq_, Y_STD), var_via_V(X_, a, th, kid, white, Xq_, Y_STD)
        out = (Xq_, Ga, Gb, va, vb)
        for arr in out:
            arr.setflags(write=False)
        _ref[case] = out
    return _ref[case]


def far_rows(case, theta):
    """What the two far points give: [y_std^2 C, 0 .., y_std^2 w]."""
    N, d, kid, white = case
    row = np.zeros(d + 1 + int(white))
    row[0] = Y_STD * Y_STD * math.exp(theta[0])
    if white:
        row[d + 1] = Y_STD * Y_STD * math.exp(theta[d + 1])
    return row


# ---------------------------------------------------------------------------------------------- the assertions
def check_closed_form(dev, case, label=""):
    """G of the device against formulation (b), column by column; returns the worst ratio deviation / bound."""
    N, d, kid, white = case
    X_, y_, a, th = load(dev, case)
    Xq_, Ga, Gb, va, vb = reference(case)
    G = dev.var_theta_grad(to_raw(case, Xq_))["G"]
    assert G.shape == (len(Xq_), d + 1 + int(white)) and np.isfinite(G).all()
    dev_j, bound = column_dev(G, Gb), column_bound(Ga, Gb)
    ratio = dev_j / bound
    colmax = np.max(np.abs(Gb), axis=0)
    print(f"var_theta_grad {label}: worst column ratio {ratio.max():.2e} (column {int(np.argmax(ratio))}), deviation per colmax "
          f"{np.max(dev_j / colmax):.2e}, a-b per colmax {np.max(np.max(np.abs(Ga - Gb), axis=0) / colmax):.2e}")
    assert np.all(dev_j <= bound), (dev_j, bound)
    # far outside: k underflows, the row is the prior's
    assert np.all(np.abs(G[-2:] - far_rows(case, th)[None, :]) <= bound), G[-2:]
    return float(ratio.max())


def check_var(dev, case, label=""):
    """var of the call against the refactorised closed form: within max(10 max|var_a - var_b|, 2 max|var_ptv - var_a|), var_ptv
    the device's own ``predict_thetas(theta_0[None], Xq, want_var=True)``; and not below minus that.  Returns the ratio."""
    N, d, kid, white = case
    X_, y_, a, th = load(dev, case)
    Xq_, Ga, Gb, va, vb = reference(case)
    Xq = to_raw(case, Xq_)
    var = dev.var_theta_grad(Xq)["var"]
    ptv = dev.predict_thetas(th[None, :], Xq, want_var=True)["var"][0]
    bound = max(10.0 * np.max(np.abs(va - vb)), 2.0 * np.max(np.abs(ptv - va)))
    dv = np.max(np.abs(var - va))
    print(f"var_theta_grad var {label}: deviation {dv:.3e}, bound {bound:.3e} (a-b {np.max(np.abs(va - vb)):.3e}, "
          f"predict_thetas_var {np.max(np.abs(ptv - va)):.3e}), ratio {dv / bound:.3f}, min var {var.min():.3e}")
    assert var.shape == (len(Xq),) and dv <= bound and np.all(var > -bound)
    assert np.array_equal(var[-2:], np.full(2, Y_STD * Y_STD * prior_var(th, d, white)))
    return float(dv / bound)


def same(a, b):
    return np.array_equal(a["G"], b["G"]) and np.array_equal(a["var"], b["var"])


def check_same_bits(dev, case, other):
    """Alone, in a batch, at any position, in split calls, on a second context; a second call repeats the first."""
    load(dev, case)
    Xq = to_raw(case, reference(case)[0])
    whole = dev.var_theta_grad(Xq)
    assert same(dev.var_theta_grad(Xq), whole)
    for i in (0, 9, len(Xq) - 1):
        one = dev.var_theta_grad(Xq[i:i + 1])
        assert np.array_equal(one["G"][0], whole["G"][i]) and one["var"][0] == whole["var"][i], i
    perm = np.random.default_rng(1).permutation(len(Xq))
    shuffled = dev.var_theta_grad(Xq[perm])
    assert np.array_equal(shuffled["G"], whole["G"][perm]) and np.array_equal(shuffled["var"], whole["var"][perm])
    a, b = dev.var_theta_grad(Xq[:11]), dev.var_theta_grad(Xq[11:])
    assert np.array_equal(np.vstack([a["G"], b["G"]]), whole["G"])
    assert np.array_equal(np.concatenate([a["var"], b["var"]]), whole["var"])
    load(other, case)
    assert same(other.var_theta_grad(Xq), whole)


def check_against_own_differences(dev, case, h=1e-4):
    """Central differences through the device's own ``predict_thetas(.., want_var=True)`` at theta +- h e_j (the fitted model
    is never touched), per column within ten times what the numpy central differences miss the numpy closed form by on the
    same model and step (floor 1e-7 of the column)."""
    N, d, kid, white = case
    X_, y_, a, th = load(dev, case)
    Xq_ = reference(case)[0][:24]                      # (without the far points: nothing to differentiate there)
    Xq = to_raw(case, Xq_)
    G = dev.var_theta_grad(Xq)["G"]
    p = len(th)
    rows = np.vstack([th[None, :] + h * np.eye(p), th[None, :] - h * np.eye(p)])
    out = dev.predict_thetas(rows, Xq, want_var=True)
    assert np.all(np.asarray(out["info"]) == 0)
    fd = ((out["var"][:p] - out["var"][p:]) / (2.0 * h)).T
    _, Gb = grad_via_V(X_, a, th, kid, white, Xq_, Y_STD)
    fd_np = central_differences(X_, a, th, kid, white, Xq_, Y_STD, h)
    colmax = np.max(np.abs(Gb), axis=0)
    bound = np.maximum(10.0 * np.max(np.abs(fd_np - Gb), axis=0), 1e-7 * colmax)
    dev_j = np.max(np.abs(G - fd), axis=0)
    print(f"var_theta_grad against the device's own differences n{N}_d{d}_k{kid}{'_w' if white else ''}: worst column ratio "
          f"{np.max(dev_j / bound):.3f}, deviation per colmax {np.max(dev_j / colmax):.2e}")
    assert np.all(dev_j <= bound), (dev_j, bound)
    return float(np.max(dev_j / bound))
