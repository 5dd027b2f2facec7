"""numpy closed form of gpry_amd/csrc/joint.hip: the joint posterior covariance, the jitter ladder, the normal variates and
the draws -- the reference of the GPU tests and, as ``NumpyJoint``, the stand-in that gives a numpy device the two calls.

``cov(Xs_, Xtrain_, theta, kid, V, y_std)``: Sigma = y_std^2 (K(X*, X*) - U^T U), U = V K*^T, from the oracle's kernel
(oracle.gpry_oracle.kernel_matrix) and the factor's ``V`` in float64; with ``dtype=np.longdouble`` the kernel entries and
both products are formed in extended precision from the same float64 coordinates, hyper-parameters and ``V`` (the error
table of profiles/joint.md: what float64 loses in the products; the factor itself is data).

``normals(seed, S, m)``: the device's variates -- Philox counter (PHASE_JOINT << 24, s, j // 2, 0), Box-Muller with the
cosine for even j and the sine for odd j (tests/tools/ns_philox.py).

``factor(Sigma, unit, jitter, dead)``: the device's ladder (eps from ``jitter``, or 1e-10 for None / a negative value;
to 1e-14 from 0, else times 100, while a pivot is not positive or l^2 <= 8 (m + 1) 2^-53 max diag; LinAlgError above 1e-4).
"""
import numpy as np

from oracle import gpry_oracle as orc
from ns_philox import philox

PHASE_JOINT = 5
MAX_POINTS, MAX_DRAWS = 4096, 65536
U53 = 2.0 ** -53


def _corr(r2, kid):
    if kid == orc.RBF:
        return np.exp(-r2 / 2)
    r = np.sqrt(r2)
    if kid == orc.MATERN12:
        return np.exp(-r)
    if kid == orc.MATERN32:
        t = r * np.sqrt(r2.dtype.type(3))
        return (1 + t) * np.exp(-t)
    t = r * np.sqrt(r2.dtype.type(5))
    return (1 + t + t * t / 3) * np.exp(-t)


def kernel(Xa_, Xb_, theta, kid, dtype=np.float64):
    """C k(|xa / l - xb / l|) for transformed coordinates; float64: the oracle's own routine."""
    if dtype == np.float64:
        return orc.kernel_matrix(np.atleast_2d(Xa_), np.asarray(theta, float), kid, Y=np.atleast_2d(Xb_))
    th = np.asarray(theta, dtype=dtype)
    C, ls = np.exp(th[0]), np.exp(th[1:])
    A, B = np.asarray(Xa_, dtype=dtype) / ls, np.asarray(Xb_, dtype=dtype) / ls
    r2 = np.zeros((len(A), len(B)), dtype=dtype)
    for k in range(A.shape[1]):
        r2 += (A[:, k, None] - B[None, :, k]) ** 2
    return C * _corr(r2, kid)


def cov(Xs_, Xtrain_, theta, kid, V, y_std=1.0, dtype=np.float64):
    Kt = kernel(Xs_, Xtrain_, theta, kid, dtype)
    U = np.asarray(V, dtype=dtype).dot(Kt.T)
    S = kernel(Xs_, Xs_, theta, kid, dtype) - U.T.dot(U)
    return (S + S.T) / 2 * dtype(y_std) ** 2


def cov_of_oracle(ref, X, dtype=np.float64):
    """Sigma of an ``OracleGPR`` at raw points X, units of y^2 (no gates)."""
    y_std = float(ref.pre_y.inverse_transform_scale(np.ones(1))[0])
    return cov(ref.pre_X.transform(np.atleast_2d(X)), ref.X_train_, ref.theta, ref.kernel_id, ref.V_, y_std, dtype)


def normals(seed, S, m):
    s, t = np.arange(S)[:, None], np.arange((m + 1) // 2)[None, :]
    ua, ub = philox(seed, PHASE_JOINT, 0, s, t, 0)
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - ua)), 6.283185307179586 * ub
    Z = np.empty((S, 2 * t.shape[1]))
    Z[:, 0::2], Z[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
    return np.ascontiguousarray(Z[:, :m])


def ladder(jitter):
    eps = 1e-10 if jitter is None or jitter < 0 else float(jitter)
    while eps <= 1e-4:
        yield eps
        eps = 1e-14 if eps == 0.0 else eps * 100.0


def factor(Sigma, unit, jitter=None, dead=None):
    """(L_c, eps) of Sigma + eps unit I with the identity on the diagonal of the ``dead`` rows."""
    m = len(Sigma)
    dead = np.zeros(m, bool) if dead is None else np.asarray(dead, bool)
    for eps in ladder(jitter):
        A = np.array(Sigma, dtype=float)
        A[np.diag_indices(m)] = np.where(dead, 1.0, np.diag(Sigma) + eps * unit)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        tol = 8.0 * (m + 1) * U53 * float(np.max(np.diag(Sigma) + eps * unit))
        if np.all(np.diag(L)[~dead] ** 2 > tol):
            return L, eps
    raise np.linalg.LinAlgError("Sigma + eps C y_std^2 I has a pivot that is not positive up to eps = 1e-4")


def draws(mu, Sigma, unit, S, seed, jitter=None, dead=None):
    """dict(Y, Z, Lc, jitter_used): Y = mu + Z L_c^T, -inf in the dead columns."""
    L, eps = factor(Sigma, unit, jitter, dead)
    Z = normals(seed, S, len(mu))
    Y = np.asarray(mu, float)[None, :] + Z.dot(L.T)
    if dead is not None:
        Y[:, np.asarray(dead, bool)] = -np.inf
    return dict(Y=Y, Z=Z, Lc=L, jitter_used=eps)


class NumpyJoint:
    """Mixin for ``tests/oracle_device.OracleDevice``: ``predict_cov`` and ``sample_joint`` of gpry_amd/_lib.Device in
    numpy (the same refusals, gates and finalisation; not the same bits)."""
    applies_gates_in_predict = False

    def _joint(self, X, mask):
        from gpry_amd._lib import GpryHipError, MASK_CLASSIFIED_INF
        X = np.ascontiguousarray(X, dtype=float)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (m, {self.d}), got {X.shape}")
        m = len(X)
        if not 1 <= m <= MAX_POINTS:
            raise GpryHipError(f"m = {m}, need 1 <= m <= {MAX_POINTS}")
        if not np.all(np.isfinite(X)):
            raise GpryHipError("a coordinate is not finite")
        if self._factor is None:
            raise GpryHipError("model not factorised")
        bits = np.zeros(m, np.uint8) if mask is None else np.asarray(mask, np.uint8).copy()
        if getattr(self, "gates", None) is not None and self.applies_gates_in_predict:
            bits |= self._gate_bits(X)
        X_ = self._to_unit(X)
        _, V, a = self._factor
        mu = kernel(X_, self.X_, self.theta, self.kid).dot(a) * self.y_std + self.y_mean
        S = cov(X_, self.X_, self.theta, self.kid, V, self.y_std)
        dead = (bits & MASK_CLASSIFIED_INF) != 0
        S[dead, :] = 0.0
        S[:, dead] = 0.0
        mean = np.minimum(mu, self.clip_hi)
        mean[bits != 0] = -np.inf
        return mu, mean, S, dead

    def predict_cov(self, X, mask=None):
        _, mean, S, _ = self._joint(X, mask)
        return dict(mean=mean, cov=S, device_ms=0.0)

    def sample_joint(self, X, S, seed, jitter=None, mask=None, want_Z=False, want_Lc=False):
        from gpry_amd._lib import GpryHipError
        mu, mean, Sig, dead = self._joint(X, mask)
        if not 1 <= int(S) <= MAX_DRAWS:
            raise GpryHipError(f"S = {S}, need 1 <= S <= {MAX_DRAWS}")
        try:
            out = draws(mu, Sig, np.exp(self.theta[0]) * self.y_std ** 2, int(S), int(seed), jitter, dead)
        except np.linalg.LinAlgError as e:
            raise GpryHipError(str(e))
        out.update(mean=mean, device_ms=0.0)
        if not want_Z:
            out["Z"] = None
        if not want_Lc:
            out["Lc"] = None
        return out
