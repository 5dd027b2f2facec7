"""numpy closed form of a GP whose kernel is ``C * (RBF | Matern) + WhiteKernel(w)``, for the white-noise tests.

With a = alpha (the per-point noise variance the regressor keeps) and w the fitted noise level:
    training matrix       K = C k(X, X) + diag(a + w)
    kernel_(X)            C k(X, X) + w I          kernel_(X, Y): no white part          kernel_.diag = C + w
    predictive variance   C + w - |V k*|^2          mean and its x-gradient: unchanged in form
    theta                 [log C, log l_1..l_d, log w],  d lml / d log w = 1/2 w (alpha_^T alpha_ - tr K^-1)
Everything else is the plain model with alpha + w, which the oracle (``oracle/gpry_oracle.py``) already evaluates.

``WhiteDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU (``oracle_device.OracleDevice`` with
the flag ``KERNEL_WHITE`` understood).  Test infrastructure only.
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky

from oracle import gpry_oracle as orc
from oracle_device import OracleDevice

KERNEL_WHITE = 0x10


def split(theta, d):
    """(theta of the product [log C, log l..], w) of a full theta [log C, log l.., log w]."""
    theta = np.asarray(theta, dtype=float)
    assert theta.shape == (d + 2,)
    return theta[:d + 1], float(np.exp(theta[d + 1]))


def kernel_train(X_, theta, kid):
    """kernel_(X_): w on the diagonal, no alpha."""
    th, w = split(theta, X_.shape[1])
    K = orc.kernel_matrix(X_, th, kid)
    K[np.diag_indices_from(K)] += w
    return K


def lml(X_, y_, alpha, theta, kid, eval_gradient=False):
    """Log marginal likelihood at the full theta; with ``eval_gradient`` also its d + 2 gradient entries."""
    th, w = split(theta, X_.shape[1])
    a = np.broadcast_to(alpha, (len(y_),)) + w
    if not eval_gradient:
        return float(orc.log_marginal_likelihood(X_, y_, a, th, kid))
    val, grad = orc.log_marginal_likelihood(X_, y_, a, th, kid, eval_gradient=True)
    if not np.isfinite(val):
        return float(val), np.zeros(len(th) + 1)
    K = orc.kernel_matrix(X_, th, kid)
    K[np.diag_indices_from(K)] += a
    L = cholesky(K, lower=True)
    al = cho_solve((L, True), y_)
    Kinv = cho_solve((L, True), np.eye(len(y_)))
    return float(val), np.append(grad, 0.5 * w * (al.dot(al) - np.trace(Kinv)))


def white_grad_from_factor(V, alpha_, w):
    """The log w entry from a fetched factor: 1/2 w (|alpha_|^2 - |V|_F^2)   (K^-1 = V^T V)."""
    return 0.5 * w * (float(np.dot(alpha_, alpha_)) - float(np.sum(V * V)))


class WhiteModel:
    """Posterior of the model at fixed theta, in the caller's units (affine maps of X and y as the device applies them)."""

    def __init__(self, X_, y_, alpha, kid, theta, x_lo=None, x_span=None, y_mean=0.0, y_std=1.0, clip_hi=np.inf):
        self.X_, self.y_, self.kid = np.asarray(X_, float), np.asarray(y_, float), int(kid)
        self.d = self.X_.shape[1]
        self.th, self.w = split(theta, self.d)
        self.C = float(np.exp(self.th[0]))
        self.alpha = np.broadcast_to(alpha, (len(self.y_),)) + self.w
        K = orc.kernel_matrix(self.X_, self.th, self.kid)
        K[np.diag_indices_from(K)] += self.alpha
        self.L, self.V, self.alpha_ = orc.factorize(K, self.y_)
        self.lo = np.zeros(self.d) if x_lo is None else np.asarray(x_lo, float)
        self.span = np.ones(self.d) if x_span is None else np.asarray(x_span, float)
        self.y_mean, self.y_std, self.clip_hi = float(y_mean), float(y_std), float(clip_hi)

    def unit(self, X):
        return (np.atleast_2d(np.asarray(X, float)) - self.lo) / self.span

    def predict(self, X):
        """(mean, std) at raw points, the mean clipped at ``clip_hi``; the white variance is part of the std."""
        X_ = self.unit(X)
        Kt = orc.kernel_matrix(X_, self.th, self.kid, Y=self.X_)
        U = self.V.dot(Kt.T)
        var = np.maximum((self.C + self.w) - np.einsum("ji,ji->i", U, U), 0.0)
        return np.minimum(Kt.dot(self.alpha_) * self.y_std + self.y_mean, self.clip_hi), np.sqrt(var) * self.y_std

    def predict_grad(self, x):
        """(mean_grad, std_grad) at one raw point with the reference's conventions (gpry/gpr.py:1236-1266): derivatives
        with respect to the TRANSFORMED coordinates, the mean's times y_std, the std's times y_std^2."""
        x_ = self.unit(x)[0]
        G = orc.kernel_gradient_x(x_, self.X_, self.th, self.kid)        # (N, d), transformed coordinates
        Kt = orc.kernel_matrix(x_[None, :], self.th, self.kid, Y=self.X_)[0]
        u = self.V.dot(Kt)
        var = (self.C + self.w) - u.dot(u)
        mean_grad = G.T.dot(self.alpha_) * self.y_std
        std_grad = -(self.V.T.dot(u)).dot(G) / np.sqrt(var) * self.y_std * self.y_std
        return mean_grad, std_grad

    def var0(self, X):
        """C + w - |u(x)|^2 in transformed units, unclamped: what a Kriging-believer session starts from."""
        Kt = orc.kernel_matrix(self.unit(X), self.th, self.kid, Y=self.X_)
        U = self.V.dot(Kt.T)
        return (self.C + self.w) - np.einsum("ji,ji->i", U, U)

    def logexp(self, X, zeta, baseline, sigma_n):
        mean, std = self.predict(X)
        with np.errstate(all="ignore"):
            return orc.logexp_f(mean, std, baseline, sigma_n, zeta)


class WhiteDevice(OracleDevice):
    """``OracleDevice`` that understands ``kernel_id | KERNEL_WHITE`` and the d + 2 theta that goes with it."""
    w = 0.0
    white = False

    @property
    def n_theta(self):
        return self.d + 1 + int(self.white)

    def set_theta(self, kernel_id, theta):
        self.white = bool(int(kernel_id) & KERNEL_WHITE)
        theta = np.array(theta, dtype=float)
        assert theta.shape == (self.n_theta,)
        self.kid, self.theta = int(kernel_id) & 0xF, theta[:self.d + 1]
        self.w = float(np.exp(theta[-1])) if self.white else 0.0
        self._factor = None

    def _shifted(self, w):
        dev = self

        class Shift:
            def __enter__(self):
                self.keep = dev.alpha
                dev.alpha = dev.alpha + w

            def __exit__(self, *exc):
                dev.alpha = self.keep
        return Shift()

    def factorize(self):
        with self._shifted(self.w):
            return OracleDevice.factorize(self)

    def lml(self, theta, eval_gradient=False):
        if not self.white:
            return OracleDevice.lml(self, theta, eval_gradient)
        self.n_lml += 1
        out = lml(self.X_, self.y_, self.alpha, theta, self.kid, eval_gradient)
        if eval_gradient:
            return out[0], out[1], int(not np.isfinite(out[0]))
        return out, int(not np.isfinite(out))

    def predict(self, X, return_std=False, mask=None):
        if not (self.white and return_std):
            return OracleDevice.predict(self, X, return_std, mask)
        from gpry_amd._lib import MASK_CLASSIFIED_INF
        mean = OracleDevice.predict(self, X, False, mask)
        L, V, a = self._factor
        U = V.dot(orc.kernel_matrix(self._to_unit(X), self.theta, self.kid, Y=self.X_).T)
        var = np.maximum((np.exp(self.theta[0]) + self.w) - np.einsum("ji,ji->i", U, U), 0.0)
        std = np.sqrt(var) * self.y_std
        if mask is not None:
            std[(np.asarray(mask, dtype=np.uint8) & MASK_CLASSIFIED_INF) != 0] = 0.0
        return mean, std

    def predict_point(self, x, mask_bits=0, want_kinv=True):
        x = np.asarray(x, dtype=float)
        mask = None if not mask_bits else np.array([mask_bits], dtype=np.uint8)
        mean, std = self.predict(x[None, :], return_std=True, mask=mask)
        mg, kg = self.predict_grad(x, want_kinv=want_kinv)
        return float(mean[0]), float(std[0]), mg, kg, int(mask_bits)

    def append_rows(self, Xnew_, ynew_, alphanew):
        keep = (self.white, self.w)
        info = OracleDevice.append_rows(self, Xnew_, ynew_, alphanew)
        assert (self.white, self.w) == keep
        return info

    def kb_register(self, X, want_var0=True):
        first, var0 = OracleDevice.kb_register(self, X, want_var0)
        return first, (None if var0 is None else var0 + self.w)
