"""numpy float64 truth of the predictive variance under a batch of thetas, the reference of the ``gpry_predict_thetas_var``
tests, and a stand-in device.

theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last; K = C phi(r) + diag(alpha [+ w]) = L L^T,
k* = C phi(r(x, X)) the cross-kernel column of a point:
    var(x) = y_std^2 (C + w - |L^-1 k*|^2)
unclamped, in untransformed units.  Two formulations:
    (a) ``var_numpy``   a triangular solve with the Cholesky factor;
    (b) ``var_via_V``   the explicit V = L^-1 and the product V k* (what the device forms).
Points are in the unit (transformed) coordinates here; the tests map them through the x-affine.

``PredictThetasVarDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU
(``predict_thetas_model.PredictThetasDevice`` whose ``predict_thetas`` accepts ``want_var``).  Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from predict_thetas_model import PredictThetasDevice
from theta_grad_model import _matrices


def prior_var(theta, d, white):
    """C + w as the device's host code forms it (libm's exp on each entry, w = 0 without a white term)."""
    return math.exp(theta[0]) + (math.exp(theta[d + 1]) if white else 0.0)


def _cross(X_, theta, kid, Xq_):
    d = X_.shape[1]
    return orc.kernel_matrix(Xq_, np.asarray(theta, dtype=float)[:d + 1], kid, Y=X_).T          # (N, M)


def var_numpy(X_, alpha, theta, kid, white, Xq_, y_std=1.0):
    """Formulation (a)."""
    theta = np.asarray(theta, dtype=float)
    K, _ = _matrices(X_, alpha, theta, kid, white)
    U = solve_triangular(cholesky(K, lower=True), _cross(X_, theta, kid, Xq_), lower=True)
    return y_std * y_std * (prior_var(theta, X_.shape[1], white) - np.einsum("ji,ji->i", U, U))


def var_via_V(X_, alpha, theta, kid, white, Xq_, y_std=1.0):
    """Formulation (b)."""
    theta = np.asarray(theta, dtype=float)
    K, _ = _matrices(X_, alpha, theta, kid, white)
    V = solve_triangular(cholesky(K, lower=True), np.eye(len(X_)), lower=True)
    U = V.dot(_cross(X_, theta, kid, Xq_))
    return y_std * y_std * (prior_var(theta, X_.shape[1], white) - np.einsum("ji,ji->i", U, U))


class PredictThetasVarDevice(PredictThetasDevice):
    """``PredictThetasDevice`` whose ``predict_thetas`` takes ``want_var``: formulation (a), one theta and one point at a
    time; a row of NaN where the matrix has no Cholesky factor.  Without the keyword the parent's answer, key for key."""
    n_ptv = 0

    def predict_thetas(self, thetas, X, want_var=False):
        out = PredictThetasDevice.predict_thetas(self, thetas, X)
        if not want_var:
            return out
        self.n_ptv += 1
        thetas = np.atleast_2d(np.asarray(thetas, dtype=float))
        Xq_ = self._to_unit(np.atleast_2d(np.asarray(X, dtype=float)))
        var = np.full(out["mean"].shape, np.nan)
        for b, th in enumerate(thetas):
            if out["info"][b] != 0:
                continue
            for i in range(len(Xq_)):
                var[b, i] = var_numpy(self.X_, self.alpha, th, self.kid, self.white, Xq_[i:i + 1], self.y_std)[0]
        out["var"] = var
        return out
