"""numpy stand-in for ``dev.hessian_mean`` (gpry_amd/_lib.py; kernel in gpry_amd/csrc/hessian.hip): gradient and Hessian
of the posterior mean in closed form from ``X_train_``, ``alpha_`` and theta in float64, the reference of the GPU tests
and the device of the CPU tests of ``laplace_gp`` and ``covmat="laplace"`` (gpry_amd/maximize.py).

With diff_j = (x_ - X_j) / l in the kernel's coordinates (x_ = (x - lo) / span under the x-affine map), r = |diff_j|,
w(r) the radial factor of the gradient and q(r) = w'(r) / r:

    RBF          w = -exp(-r^2/2)                         q = exp(-r^2/2)
    Matern 3/2   w = -3 exp(-sqrt3 r)                     q = 3 sqrt3 exp(-sqrt3 r) / r   (0 at r = 0)
    Matern 5/2   w = -(5/3) (1 + sqrt5 r) exp(-sqrt5 r)   q = (25/3) exp(-sqrt5 r)

    g_a  = y_std C sum_j alpha_j w_j diff_ja / (l_a span_a)
    H_ab = y_std C (sum_j alpha_j q_j diff_ja diff_jb + delta_ab sum_j alpha_j w_j) / (l_a l_b span_a span_b)

in raw coordinates and units of y (span = 1 without the map): of the unclipped, ungated mean.  Matern 1/2 has no
Hessian at the training rows and raises ValueError.  H is returned exactly symmetric (the lower triangle, mirrored)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maximize_numpy import HostGpr, MaxNumpyDevice  # noqa: E402

RBF, M12, M32, M52 = range(4)


class MeanDerivatives:
    """The closed form.  X_train_: the training rows in the kernel's coordinates; x_lo / x_span: the x-affine map (None:
    there is none); y_std: the scale of the y-normalisation (1 without one)."""

    def __init__(self, X_train_, alpha_, theta, kernel_id, x_lo=None, x_span=None, y_std=1.0):
        if kernel_id == M12:
            raise ValueError("the mean of a Matern-1/2 model is not differentiable at the training rows; it has no Hessian")
        self.Xt = np.asarray(X_train_, dtype=float)
        self.alpha = np.asarray(alpha_, dtype=float).ravel()
        theta = np.asarray(theta, dtype=float)
        self.d = d = self.Xt.shape[1]
        self.C, self.ls = float(np.exp(theta[0])), np.broadcast_to(np.exp(theta[1:]), (d,)).astype(float)
        self.kid = kernel_id
        self.x_lo = np.zeros(d) if x_lo is None else np.asarray(x_lo, dtype=float)
        self.x_span = np.ones(d) if x_span is None else np.asarray(x_span, dtype=float)
        self.y_std = float(y_std)

    @classmethod
    def of_oracle(cls, ref):
        """From an ``oracle.gpry_oracle.OracleGPR`` with its model up to date."""
        lo = getattr(ref.pre_X, "lo", None)
        span = None if lo is None else ref.pre_X.hi - ref.pre_X.lo
        return cls(ref.X_train_, ref.alpha_, ref.theta, ref.kernel_id, lo, span, ref.pre_y.inverse_transform_scale(1.0))

    def terms(self, x):
        """(diff (N, d), alpha w (N,), alpha q (N,)) of one point: the summands of g and H before their scalings."""
        diff = ((x - self.x_lo) / self.x_span - self.Xt) / self.ls
        r2 = np.sum(diff ** 2, axis=1)
        r = np.sqrt(r2)
        if self.kid == RBF:
            q = np.exp(-0.5 * r2)
            w = -q
        elif self.kid == M32:
            e = np.exp(-np.sqrt(3.0) * r)
            w = -3.0 * e
            q = np.zeros_like(r)
            nz = r != 0
            q[nz] = 3.0 * np.sqrt(3.0) * e[nz] / r[nz]
        else:
            e = np.exp(-np.sqrt(5.0) * r)
            w = -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * e
            q = (25.0 / 3.0) * e
        return diff, self.alpha * w, self.alpha * q

    def scale(self):
        """y_std C and l span: g = scale[0] (aw @ diff) / scale[1]."""
        return self.y_std * self.C, self.ls * self.x_span

    def _one(self, x):
        diff, aw, aq = self.terms(x)
        f = self.ls * self.x_span
        g = self.y_std * self.C * (aw @ diff) / f
        S = (diff * aq[:, None]).T @ diff + np.sum(aw) * np.eye(self.d)
        H = self.y_std * self.C * S / np.outer(f, f)
        L = np.tril(H)
        return g, L + np.tril(H, -1).T

    def grad_hess(self, X):
        """(g (n, d), H (n, d, d)) at the rows of X (raw coordinates)."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        out = [self._one(x) for x in X]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


class HessNumpyDevice(MaxNumpyDevice):
    """``MaxNumpyDevice`` (``maximize_mean``) with the device's ``hessian_mean(X) -> {"y", "g", "H", "device_ms"}``: y from
    ``loglike`` (clip and gates included), g and H from ``deriv`` (a ``MeanDerivatives``, or anything with its
    ``grad_hess``).  ``hess_calls`` keeps the points of every call."""

    def __init__(self, loglike, grad_x, deriv):
        super().__init__(loglike, grad_x)
        self.deriv = deriv
        self.hess_calls = []

    def hessian_mean(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.ndim != 2 or len(X) < 1 or not np.all(np.isfinite(X)):
            raise ValueError(f"hessian_mean: finite points of shape (npts >= 1, d) are needed, got {X.shape}")
        self.hess_calls.append(X.copy())
        g, H = self.deriv.grad_hess(X)
        return dict(y=np.asarray(self.loglike(X), dtype=float), g=g, H=H, device_ms=0.0)


class QuadraticDerivatives:
    """grad_hess of y = y0 - (x - mu)^T A (x - mu) / 2 for a symmetric A (not necessarily positive definite)."""

    def __init__(self, mu, A, y0=0.0):
        self.mu, self.A, self.y0 = np.asarray(mu, dtype=float), np.asarray(A, dtype=float), float(y0)

    def value(self, X):
        D = np.atleast_2d(X) - self.mu
        return self.y0 - 0.5 * np.einsum("ia,ab,ib->i", D, self.A, D)

    def grad(self, X):
        return -(np.atleast_2d(X) - self.mu) @ self.A

    def grad_hess(self, X):
        X = np.atleast_2d(X)
        return self.grad(X), np.repeat(-self.A[None], len(X), axis=0)


def quadratic_gpr(mu, A, bounds, X_train, y0=0.0):
    """A ``HostGpr`` whose surrogate is the quadratic form above, on a ``HessNumpyDevice``."""
    q = QuadraticDerivatives(mu, A, y0)
    X_train = np.asarray(X_train, dtype=float)
    return HostGpr(HessNumpyDevice(q.value, q.grad, q), X_train, q.value(X_train), bounds), q


def oracle_gpr(model):
    """(oracle-side ``HostGpr`` on a ``HessNumpyDevice``, its ``MeanDerivatives``) of a ``sampler_walk.Model``."""
    from hmc_numpy import oracle_grad_x
    ref = model.oracle()
    mean = model.mean_fn(ref)
    clip = float(ref.clip_hi())
    deriv = MeanDerivatives.of_oracle(ref)
    dev = HessNumpyDevice(lambda X: np.minimum(mean(X), clip), oracle_grad_x(ref), deriv)
    gpr = HostGpr(dev, model.X, model.y, model.bounds)
    gpr.kernel_id = model.kid
    return gpr, deriv
