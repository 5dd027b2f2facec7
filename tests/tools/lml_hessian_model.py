"""numpy float64 closed form of the Hessian of a GP's log marginal likelihood in theta, the reference of the
``gpry_lml_hessian`` tests.

With K = C k(r^2) + diag(alpha [+ w]), alpha_ = K^-1 y_, W = alpha_ alpha_^T - K^-1, K_i = dK / dtheta_i and
K_ij = d2K / dtheta_i dtheta_j, theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last:
    H_ij = 1/2 tr(W K_ij) - (K_i alpha_)^T K^-1 (K_j alpha_) + 1/2 tr(K^-1 K_i K^-1 K_j)
    K_00 = K_0, K_0i = K_i, K_ww = w I, every other entry with log w zero (also (log C, log w));
    K_ij = C (g D_i D_j - 2 delta_ij h D_i) for two length scales, g = -2 dh / dr^2, 0 at r = 0.
Two formulations:
    (a) ``hessian_explicit``  explicit inverse, B_i = K^-1 K_i, the formula as it stands;
    (b) ``hessian_via_V``     V = L^-1: A_i = V K_i V^T, tr(K^-1 K_i K^-1 K_j) = <A_i, A_j>, middle = (V K_i alpha_) . (V K_j alpha_).
Both return ``(lml, grad, H)``, ``(-inf, zeros, zeros)`` where K has no Cholesky factor.

``HessDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU (``loo_fit_model.LooDevice`` with
``lml_hessian``).  Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from loo_fit_model import LooDevice, _matrices, problem  # noqa: F401


def second_weight(X_, theta, kid):
    """(C g, D): the weight of D_i D_j in d2K / dlog l_i dlog l_j, zero at r = 0, and D (N, N, d)."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    Xs = X_ / np.exp(theta[1:d + 1])
    D = (Xs[:, None, :] - Xs[None, :, :]) ** 2
    r2 = D.sum(axis=2)
    r = np.sqrt(r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kid == orc.RBF:
            g = np.exp(-0.5 * r2)
        elif kid == orc.MATERN12:
            g = np.exp(-r) * (1.0 + r) / r ** 3
        elif kid == orc.MATERN32:
            t = math.sqrt(3.0) * r
            g = 9.0 * np.exp(-t) / t
        else:
            t = math.sqrt(5.0) * r
            g = (25.0 / 3.0) * np.exp(-t)
    g = np.where(r2 > 0.0, g, 0.0)
    return math.exp(theta[0]) * g, D


def second_derivatives(X_, theta, kid, white, dKs):
    """K_ij for i <= j as a dict; entries that are zero matrices are left out."""
    d = X_.shape[1]
    Cg, D = second_weight(X_, theta, kid)
    K2 = {}
    for j in range(d + 1):
        K2[(0, j)] = dKs[j]
    for i in range(1, d + 1):
        for j in range(i, d + 1):
            M = Cg * D[:, :, i - 1] * D[:, :, j - 1]
            if i == j:
                M = M - 2.0 * dKs[i]
            K2[(i, j)] = M
    if white:
        K2[(d + 1, d + 1)] = dKs[d + 1]
    return K2


def _failed(p):
    return -np.inf, np.zeros(p), np.zeros((p, p))


def _assemble(p, first, middle, trace):
    H = np.zeros((p, p))
    for i in range(p):
        for j in range(i, p):
            H[i, j] = H[j, i] = first(i, j) - middle(i, j) + 0.5 * trace(i, j)
    return H


def hessian_explicit(X_, y_, alpha, theta, kid, white=False):
    """Formulation (a)."""
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    p, N = len(dKs), len(y_)
    try:
        L = cholesky(K, lower=True)
    except np.linalg.LinAlgError:
        return _failed(p)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    al = Kinv.dot(y_)
    W = np.outer(al, al) - Kinv
    lml = -0.5 * y_.dot(al) - np.sum(np.log(np.diag(L))) - 0.5 * N * math.log(2.0 * math.pi)
    grad = np.array([0.5 * np.sum(W * dK) for dK in dKs])
    K2 = second_derivatives(X_, theta, kid, white, dKs)
    B = [Kinv.dot(dK) for dK in dKs]
    Ka = [dK.dot(al) for dK in dKs]
    H = _assemble(p, lambda i, j: 0.5 * np.sum(W * K2[(i, j)]) if (i, j) in K2 else 0.0,
                  lambda i, j: Ka[i].dot(Kinv.dot(Ka[j])), lambda i, j: np.sum(B[i] * B[j].T))
    return lml, grad, H


def hessian_via_V(X_, y_, alpha, theta, kid, white=False):
    """Formulation (b)."""
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    p, N = len(dKs), len(y_)
    try:
        L = cholesky(K, lower=True)
    except np.linalg.LinAlgError:
        return _failed(p)
    V = solve_triangular(L, np.eye(N), lower=True)
    z = V.dot(y_)
    al = V.T.dot(z)
    W = np.outer(al, al) - V.T.dot(V)
    lml = -0.5 * z.dot(z) - np.sum(np.log(np.diag(L))) - 0.5 * N * math.log(2.0 * math.pi)
    grad = np.array([0.5 * np.sum(W * dK) for dK in dKs])
    K2 = second_derivatives(X_, theta, kid, white, dKs)
    A = [V.dot(dK).dot(V.T) for dK in dKs]
    u = [V.dot(dK.dot(al)) for dK in dKs]
    H = _assemble(p, lambda i, j: 0.5 * np.sum(W * K2[(i, j)]) if (i, j) in K2 else 0.0,
                  lambda i, j: u[i].dot(u[j]), lambda i, j: np.sum(A[i] * A[j]))
    return lml, grad, H


class HessDevice(LooDevice):
    """``LooDevice`` with ``lml_hessian`` (formulation (b)); counts its calls."""
    n_hess = 0

    def lml_hessian(self, theta):
        self.n_hess += 1
        theta = np.asarray(theta, dtype=float)
        assert theta.shape == (self.n_theta,)
        lml, grad, H = hessian_via_V(self.X_, self.y_, self.alpha, theta, self.kid, self.white)
        return {"lml": lml, "grad": grad, "H": H, "info": int(not np.isfinite(lml)), "device_ms": 0.0}
