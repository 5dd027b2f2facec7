"""numpy float64 truth of the posterior mean under a batch of thetas, the reference of the ``gpry_predict_thetas`` tests, and
a stand-in device.

theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last; K = C phi(r) + diag(alpha [+ w]),
alpha_ = K^-1 y_, mean(x) = y_mean + y_std k(x)^T alpha_ -- unclipped and ungated.  Two formulations:
    (a) ``theta_grad_model.mean_numpy``   two triangular solves with the Cholesky factor;
    (b) ``mean_via_V``                    the explicit V = L^-1 and alpha_ = V^T (V y_) (what the device's chain forms).
Points are in the unit (transformed) coordinates here; the tests map them through the x-affine.

``PredictThetasDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU
(``theta_grad_model.ThetaGradDevice`` with ``predict_thetas``).  Test infrastructure only.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from theta_grad_model import (ThetaGradDevice, W_FLAG, Y_MEAN, Y_STD, _matrices, affine, load, mean_numpy,  # noqa: F401
                              points, problem, to_raw)

# (N, d, kernel id, white): what each shape exercises is said in tests/test_predict_thetas_gpu.py
CASES = ([(50, 1, 1, False)] + [(130, 2, kid, white) for kid in range(4) for white in (False, True)]
         + [(333, 5, 2, True), (300, 17, 2, True), (256, 32, 0, False), (1100, 8, 3, True), (2500, 4, 1, False)])
IDS = [f"n{N}_d{d}_k{kid}{'_w' if white else ''}" for N, d, kid, white in CASES]


def mean_via_V(X_, y_, alpha, theta, kid, white, Xq_, y_mean=0.0, y_std=1.0):
    """Formulation (b)."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    K, _ = _matrices(X_, alpha, theta, kid, white)
    V = solve_triangular(cholesky(K, lower=True), np.eye(len(y_)), lower=True)
    al = V.T.dot(V.dot(y_))
    return y_mean + y_std * orc.kernel_matrix(Xq_, theta[:d + 1], kid, Y=X_).dot(al)


def thetas_of(case, theta, n=4, step=0.3, seed=11):
    """The rows of the tests: the model's theta as row 0, then ``n`` rows at theta + step N(0, 1) from a fixed seed."""
    rng = np.random.default_rng(seed + 13 * case[0] + case[1])
    return np.vstack([theta[None, :], theta[None, :] + step * rng.standard_normal((n, len(theta)))])


class PredictThetasDevice(ThetaGradDevice):
    """``ThetaGradDevice`` with ``predict_thetas``: formulation (a), one theta and one point at a time, so that -- as on the
    device -- a value's bits do not depend on the batch it comes in; ``-inf`` / NaN / ``info = 1`` where the matrix has no
    Cholesky factor.  ``lml_fn`` (theta -> value), when set, replaces the log marginal likelihood it reports."""
    n_pt = 0
    lml_fn = None

    def predict_thetas(self, thetas, X):
        self.n_pt += 1
        thetas = np.atleast_2d(np.asarray(thetas, dtype=float))
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if thetas.shape[1] != self.n_theta:
            raise ValueError(f"expected {self.n_theta} columns, got {thetas.shape[1]}")
        if X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        assert len(X) >= 1 and np.all(np.isfinite(X)) and np.all(np.isfinite(thetas))
        Xq_ = self._to_unit(X)
        B, M = len(thetas), len(X)
        mean, lml, info = np.full((B, M), np.nan), np.full(B, -np.inf), np.zeros(B, dtype=np.int32)
        for b, th in enumerate(thetas):
            try:
                for i in range(M):
                    mean[b, i] = mean_numpy(self.X_, self.y_, self.alpha, th, self.kid, self.white, Xq_[i:i + 1], self.y_mean,
                                            self.y_std)[0]
            except np.linalg.LinAlgError:
                mean[b], info[b] = np.nan, 1
                continue
            lml[b] = self.lml_fn(th) if self.lml_fn is not None else self.lml(th, False)[0]
        return {"mean": mean, "lml": lml, "info": info, "device_ms": 0.0}
