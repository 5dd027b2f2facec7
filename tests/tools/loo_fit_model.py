"""numpy float64 closed form of the leave-one-out log predictive density of a GP's training targets and its theta-gradient
(Rasmussen & Williams section 5.4.2), the reference of the ``gpry_loo_objective`` tests.

With K = C k(X, X) + diag(alpha [+ w]), alpha_ = K^-1 y_ and q_i = (K^-1)_ii, in transformed units:
    L(theta) = sum_i [ 1/2 log q_i - alpha_i^2 / (2 q_i) ] - N/2 log 2 pi
Two formulations of the gradient:
    (a) ``loo_explicit``   explicit inverse, R&W eq. 5.13 one hyper-parameter at a time:
                           Z_j = K^-1 dK_j,  dL/dtheta_j = sum_i [ alpha_i (Z_j alpha_)_i - 1/2 (1 + alpha_i^2 / q_i) (Z_j K^-1)_ii ] / q_i
    (b) ``loo_one_product`` Cholesky / V = L^-1 route, the sum over i taken before the contraction:
                           c_i = -1/2 (1 + alpha_i^2 / q_i) / q_i,  b = K^-1 (alpha_ / q),  H = diag(sqrt(-c)) K^-1,
                           dL/dtheta_j = sum_kl [ 1/2 (b alpha_^T + alpha_ b^T) - H^T H ]_kl (dK_j)_kl
theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last (dK / d log w = w I).

``LooDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU (``white_model.WhiteDevice`` with
``loo_objective``).  Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from white_model import WhiteDevice


def _matrices(X_, alpha, theta, kid, white):
    """K with the noise on its diagonal and the list of dK / d theta_j."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    assert theta.shape == (d + 1 + int(white),)
    K, dK = orc.kernel_matrix(X_, theta[:d + 1], kid, eval_gradient=True)
    w = math.exp(theta[d + 1]) if white else 0.0
    K[np.diag_indices_from(K)] += np.broadcast_to(alpha, (len(X_),)) + w
    dKs = [dK[:, :, j] for j in range(d + 1)]
    if white:
        dKs.append(w * np.eye(len(X_)))
    return K, dKs


def _value(al, q):
    return float(np.sum(0.5 * np.log(q) - 0.5 * al * al / q) - 0.5 * len(q) * math.log(2.0 * math.pi))


def loo_explicit(X_, y_, alpha, theta, kid, white=False, eval_gradient=True):
    """Formulation (a)."""
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    try:
        cholesky(K, lower=True)
    except np.linalg.LinAlgError:
        return (-np.inf, np.zeros(len(dKs))) if eval_gradient else -np.inf
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    al, q = Kinv.dot(y_), np.diag(Kinv).copy()
    val = _value(al, q)
    if not eval_gradient:
        return val
    grad = np.empty(len(dKs))
    for j, dK in enumerate(dKs):
        Z = Kinv.dot(dK)
        grad[j] = np.sum((al * Z.dot(al) - 0.5 * (1.0 + al * al / q) * np.einsum("ik,ki->i", Z, Kinv)) / q)
    return val, grad


def loo_one_product(X_, y_, alpha, theta, kid, white=False, eval_gradient=True):
    """Formulation (b): what the device computes, in numpy."""
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    try:
        L = cholesky(K, lower=True)
    except np.linalg.LinAlgError:
        return (-np.inf, np.zeros(len(dKs))) if eval_gradient else -np.inf
    V = solve_triangular(L, np.eye(len(y_)), lower=True)
    al = V.T.dot(V.dot(y_))
    q = np.einsum("ki,ki->i", V, V)
    val = _value(al, q)
    if not eval_gradient:
        return val
    Kinv = V.T.dot(V)
    c = -0.5 * (1.0 + al * al / q) / q
    b = Kinv.dot(al / q)
    H = np.sqrt(-c)[:, None] * Kinv
    Wp = 0.5 * (np.outer(b, al) + np.outer(al, b)) - H.T.dot(H)
    return val, np.array([np.sum(Wp * dK) for dK in dKs])


def loo_terms(X_, y_, alpha, theta, kid, white=False):
    """(alpha_, q) of the model."""
    K, _ = _matrices(X_, alpha, theta, kid, white)
    Kinv = np.linalg.inv(K)
    return Kinv.dot(y_), np.diag(Kinv).copy()


def sqdist_extended(A, B, ls):
    """Squared distances of the rows of ``A`` and ``B`` scaled by the length scales ``ls``, all ``np.longdouble``."""
    As, Bs = A / ls, B / ls
    r2 = np.zeros((len(A), len(B)), dtype=np.longdouble)
    for k in range(A.shape[1]):
        df = As[:, None, k] - Bs[None, :, k]
        r2 += df * df
    return r2


def corr_extended(r2, kid):
    """The correlation from the scaled squared distance in ``np.longdouble``."""
    ld = np.longdouble
    if kid == orc.RBF:
        return np.exp(-r2 / 2)
    t = np.sqrt(r2) * np.sqrt(ld(2 * orc._NU[kid]))
    poly = {orc.MATERN12: 1, orc.MATERN32: 1 + t, orc.MATERN52: 1 + t + t * t / 3}[kid]
    return poly * np.exp(-t)


def factor_extended(X_, alpha, theta, kid, white=False):
    """(K, L, V = L^-1) of the training matrix in numpy's extended precision: the kernel matrix, the Cholesky factor column
    by column and its inverse row by row, all in ``np.longdouble``.  ``None`` where a pivot is not positive."""
    ld = np.longdouble
    X = np.asarray(X_, dtype=ld)
    theta = np.asarray(theta, dtype=ld)
    N, d = X.shape
    K = np.exp(theta[0]) * corr_extended(sqdist_extended(X, X, np.exp(theta[1:d + 1])), kid)
    K[np.diag_indices(N)] = np.exp(theta[0]) + np.asarray(np.broadcast_to(alpha, (N,)), dtype=ld) \
        + (np.exp(theta[d + 1]) if white else ld(0))
    L = np.zeros((N, N), dtype=ld)
    for j in range(N):                              # Cholesky, column by column
        s = K[j, j] - L[j, :j].dot(L[j, :j])
        if not s > 0:
            return None
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    V = np.zeros((N, N), dtype=ld)
    for i in range(N):                              # V = L^-1, row by row
        V[i, :i] = -L[i, :i].dot(V[:i, :i]) / L[i, i]
        V[i, i] = 1 / L[i, i]
    return K, L, V


def value_extended(X_, y_, alpha, theta, kid, white=False):
    """The value alone in numpy's extended precision (``factor_extended``), for the central differences: a float64 value
    carries a rounding error of about 1e-16 cond(K) of its size, which a step of 1e-6 turns into 1e-10 cond(K) of the
    gradient -- above 1e-5 on the models without a white term (cond 5e5 .. 1e6)."""
    ld = np.longdouble
    K, L, V = factor_extended(X_, alpha, theta, kid, white)
    N = len(V)
    al = V.T.dot(V.dot(np.asarray(y_, dtype=ld)))
    q = np.einsum("ki,ki->i", V, V)
    return np.sum(np.log(q) / 2 - al * al / q / 2) - ld(N) / 2 * np.log(2 * ld(np.pi))


def central_differences(X_, y_, alpha, theta, kid, white=False, h=1e-6):
    """Central differences of ``value_extended`` with step ``h`` (truncation O(h^2))."""
    theta = np.asarray(theta, dtype=float)
    g = np.empty(len(theta))
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        g[j] = float((value_extended(X_, y_, alpha, theta + e, kid, white)
                      - value_extended(X_, y_, alpha, theta - e, kid, white)) / (2.0 * h))
    return g


def problem(N, d, seed, white):
    """The models of the tests: uniform X in the unit cube with row 1 a copy of row 0 (the r = 0 branch of the Matern
    derivatives), y_ = standardised sin(3 sum x) + 0.05 noise, alpha = 1e-4, theta = log [2, l ~ U(0.2, 0.6)] and
    w = 1e-3 where a white term is present."""
    rng = np.random.default_rng(seed)
    X_ = rng.uniform(0, 1, (N, d))
    X_[1] = X_[0]
    y = np.sin(3 * X_.sum(1)) + 0.05 * rng.standard_normal(N)
    y_ = (y - y.mean()) / y.std()
    theta = np.log(np.append(2.0, rng.uniform(0.2, 0.6, d)))
    if white:
        theta = np.append(theta, math.log(1e-3))
    return X_, y_, np.full(N, 1e-4), theta


class LooDevice(WhiteDevice):
    """``WhiteDevice`` with the leave-one-out objective (formulation (b)); counts its calls."""
    n_loo = 0

    def loo_objective(self, theta, eval_gradient=False):
        self.n_loo += 1
        theta = np.asarray(theta, dtype=float)
        assert theta.shape == (self.n_theta,)
        out = loo_one_product(self.X_, self.y_, self.alpha, theta, self.kid, self.white, eval_gradient)
        if eval_gradient:
            return out[0], out[1], int(not np.isfinite(out[0]))
        return out, int(not np.isfinite(out))
