"""numpy float64 truth of ``gpry_predict_without``: what a GP predicts without a group G of its training points, as a change
against the full model at the same theta, y map and noise, and a stand-in device.

K = C phi(r) + diag(alpha [+ w]) = L L^T, alpha_ = K^-1 y_, k* the cross-kernel column of a point.  Two formulations:
    (a) ``refit``      remove the rows, Cholesky of the reduced matrix, predict, subtract the full model's prediction;
    (b) ``downdate``   from the full factor: V = L^-1, B = V_G^T V_G = L_B L_B^T, W = L_B^-1, t = W alpha_G, S = W (V_G^T V),
                       s = S k*:   dmean = -y_std s.t,   dvar = +y_std^2 |s|^2   (what the device forms).
Both return (dmean, dvar), each (M,), in untransformed units; the prior variance and y_mean cancel.  Points are in the unit
(transformed) coordinates here; the tests map them through the x-affine.

``groups_of`` lists the groups of the device tests.  ``NumpyWithout`` is the mixin that gives tests/oracle_device.OracleDevice
the call for the tests without a GPU.  Test infrastructure only.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import loo_numpy as ln
from oracle import gpry_oracle as orc
from theta_grad_model import _matrices

GROUP_BATCH_ROWS = 1024     # predict_without.hip: PW_ROWS, stacked padded rows of one internal batch of groups
PANEL_POINTS = 2048         # ... PW_PC, points per panel
UPLOAD_POINTS = 32768       # ... PW_XC, points per upload


def _cross(X_, theta, kid, Xq_):
    d = X_.shape[1]
    return orc.kernel_matrix(Xq_, np.asarray(theta, dtype=float)[:d + 1], kid, Y=X_).T          # (N, M)


def full_model(K, y_, ks, y_std=1.0):
    """(y_std k*^T alpha_, y_std^2 |L^-1 k*|^2) of the matrix K: the mean without y_mean, the explained variance."""
    L = cholesky(K, lower=True)
    al = solve_triangular(L, solve_triangular(L, y_, lower=True), lower=True, trans=1)
    U = solve_triangular(L, ks, lower=True)
    return y_std * ks.T.dot(al), y_std * y_std * np.einsum("ji,ji->i", U, U)


def refit_K(K, y_, ks, group, y_std=1.0):
    """Formulation (a) on a given matrix and cross-kernel block ks (N, M)."""
    keep = np.setdiff1d(np.arange(len(y_)), np.asarray(group))
    m0, e0 = full_model(K, y_, ks, y_std)
    m1, e1 = full_model(K[np.ix_(keep, keep)], y_[keep], ks[keep], y_std)
    return m1 - m0, e0 - e1


def downdate_V(V, alpha_, ks, group, y_std=1.0):
    """Formulation (b) from V = L^-1 and alpha_ = K^-1 y_."""
    g = np.sort(np.asarray(group))
    VG = V[:, g]
    W = solve_triangular(cholesky(VG.T.dot(VG), lower=True), np.eye(len(g)), lower=True)
    t = W.dot(alpha_[g])
    s = W.dot(VG.T.dot(V)).dot(ks)                      # (n, M)
    return -y_std * t.dot(s), y_std * y_std * np.einsum("ai,ai->i", s, s)


def refit(X_, y_, alpha, theta, kid, white, group, Xq_, y_std=1.0):
    """Formulation (a)."""
    K, _ = _matrices(X_, alpha, np.asarray(theta, dtype=float), kid, white)
    return refit_K(K, y_, _cross(X_, theta, kid, Xq_), group, y_std)


def downdate(X_, y_, alpha, theta, kid, white, group, Xq_, y_std=1.0):
    """Formulation (b)."""
    K, _ = _matrices(X_, alpha, np.asarray(theta, dtype=float), kid, white)
    V = solve_triangular(cholesky(K, lower=True), np.eye(len(y_)), lower=True)
    return downdate_V(V, V.T.dot(V.dot(y_)), _cross(X_, theta, kid, Xq_), group, y_std)


def groups_of(N, seed=3):
    """The groups of a device case of N >= 50 rows, by name, in the order of the call."""
    rng = np.random.default_rng(seed + N)
    five = np.array([N - 1, 7, 0, N // 2, 3])
    sixteen = np.arange(N - 16, N)
    return [("first", np.array([0])), ("last", np.array([N - 1])), ("five_unsorted", five), ("last16", sixteen),
            ("seventeen", rng.choice(N, 17, replace=False)), ("sixtyfour", rng.choice(N, min(64, N - 2), replace=False)),
            ("overlap_a", np.arange(10, 22)), ("overlap_b", np.arange(16, 30)), ("last16_again", sixteen.copy())]


class NumpyWithout:
    """Mixin for ``tests/oracle_device.OracleDevice``: ``predict_without`` of gpry_amd/_lib.Device in numpy, formulation
    (b) from the factor the device holds, one group and one point at a time (the same refusals and units; not the same
    bits).  Counts its calls."""
    n_pw = 0

    def predict_without(self, groups, X, want=("dmean", "dvar")):
        from gpry_amd._lib import GpryHipError
        self.n_pw += 1
        if self._factor is None:
            raise GpryHipError("the context holds no valid factor")
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        try:
            groups = ln.check_groups(groups, self.N)
        except ValueError as e:
            raise GpryHipError(str(e))
        if len(X) < 1 or not np.all(np.isfinite(X)):
            raise GpryHipError("M < 1 or a coordinate that is not finite")
        V, a = self._factor[1], self._factor[2]
        ks = orc.kernel_matrix(self._to_unit(X), self.theta, self.kid, Y=self.X_).T
        dm, dv = np.empty((len(groups), len(X))), np.empty((len(groups), len(X)))
        info = np.zeros(len(groups), dtype=np.int32)
        for k, g in enumerate(groups):
            try:
                for i in range(len(X)):
                    m, v = downdate_V(V, a, ks[:, i:i + 1], g, self.y_std)
                    dm[k, i], dv[k, i] = m[0], v[0]
            except np.linalg.LinAlgError:
                dm[k], dv[k], info[k] = np.nan, np.nan, 1
        return {"dmean": dm if "dmean" in want else None, "dvar": dv if "dvar" in want else None, "info": info,
                "device_ms": 0.0}
