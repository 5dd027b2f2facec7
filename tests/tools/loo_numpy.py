"""numpy closed forms of gpry_amd/csrc/loo.hip: leave-one-out, leave-group-out and one-step-ahead predictives of the
training targets from the factor's ``V = L^-1`` and ``alpha_ = K^-1 y_`` (Rasmussen & Williams 5.4.2) -- the reference of
the GPU tests and, as ``NumpyLoo``, the stand-in that gives a numpy device the two calls -- and the brute-force refits
(rows and columns of K deleted, the rest solved) that the closed forms are checked against.

Everything is formed in transformed space and mapped to units of y at the end: mean -> mean y_std + y_mean,
variance -> variance y_std^2.  ``noise`` is the vector the device calls ``alpha``: sigma_n^2 per point, transformed units.
"""
import numpy as np

MAX_GROUP = 64
LOG_2PI = float(np.log(2.0 * np.pi))


def q_and_w(V, y_):
    """q_i = (K^-1)_ii = sum_k V_ki^2 and w = V y_ (lower triangular V)."""
    V = np.tril(np.asarray(V, dtype=float))
    return np.einsum("ki,ki->i", V, V), V.dot(np.asarray(y_, dtype=float))


def loo(V, alpha_, y_, noise, y_mean=0.0, y_std=1.0):
    """The outputs of ``Device.loo`` (plus ``q``, ``w`` and ``vdiag``) from the factor."""
    V, y_, alpha_ = np.asarray(V, dtype=float), np.asarray(y_, dtype=float), np.asarray(alpha_, dtype=float)
    noise = np.broadcast_to(np.asarray(noise, dtype=float), y_.shape)
    q, w = q_and_w(V, y_)
    vd = np.diag(V).copy()
    ys2 = float(y_std) ** 2
    return dict(q=q, w=w, vdiag=vd,
                mean=(y_ - alpha_ / q) * y_std + y_mean, var_y=ys2 / q, var_f=np.maximum(1.0 / q - noise, 0.0) * ys2,
                seq_mean=(y_ - w / vd) * y_std + y_mean, seq_var_y=ys2 / vd ** 2, device_ms=0.0)


def check_groups(groups, N):
    """The groups as int64 arrays; ValueError with the device's four refusals."""
    groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    if len(groups) < 1:
        raise ValueError("ngroups = 0, need 1 <= ngroups")
    for k, g in enumerate(groups):
        if len(g) < 1:
            raise ValueError(f"group {k} is empty")
        if len(g) > MAX_GROUP:
            raise ValueError(f"group {k} has {len(g)} points, at most {MAX_GROUP}")
        if g.min() < 0 or g.max() >= N:
            raise ValueError(f"an index of group {k} is outside [0, {N})")
        if len(np.unique(g)) != len(g):
            raise ValueError(f"group {k} holds an index more than once")
    return groups


def leave_out(V, alpha_, y_, groups, y_mean=0.0, y_std=1.0):
    """The outputs of ``Device.leave_out`` from the factor: B = V[:, G]^T V[:, G], delta = B^-1 alpha_G."""
    V, y_, alpha_ = np.tril(np.asarray(V, dtype=float)), np.asarray(y_, dtype=float), np.asarray(alpha_, dtype=float)
    groups = check_groups(groups, len(y_))
    ng = len(groups)
    out = dict(mean=[], cov=[], chi2=np.empty(ng), logpdf=np.empty(ng), info=np.zeros(ng, dtype=np.int32),
               dof=np.array([len(g) for g in groups], dtype=np.int64), device_ms=0.0)
    for k, g in enumerate(groups):
        n = len(g)
        VG = V[:, g]
        B = VG.T.dot(VG)
        try:
            L = np.linalg.cholesky(B)
            if not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0):
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            out["mean"].append(np.full(n, np.nan))
            out["cov"].append(np.full((n, n), np.nan))
            out["chi2"][k] = out["logpdf"][k] = np.nan
            out["info"][k] = 1
            continue
        W = np.linalg.solve(L, np.eye(n))
        cov = W.T.dot(W)
        delta = cov.dot(alpha_[g])
        chi2 = float(alpha_[g].dot(delta))
        out["mean"].append((y_[g] - delta) * y_std + y_mean)
        out["cov"].append((cov + cov.T) / 2 * float(y_std) ** 2)
        out["chi2"][k] = chi2
        out["logpdf"][k] = -0.5 * chi2 + np.log(np.diag(L)).sum() - n * (0.5 * LOG_2PI + np.log(y_std))
    return out


# ---- brute force: the model refitted without the points, theta and pre-processors frozen ----------------------------
def brute_leave_out(K, y_, group, y_mean=0.0, y_std=1.0):
    """(mean, cov) of the OBSERVATIONS y_G predicted by the model of the other rows; ``K`` = C k(X_, X_) + diag(noise)."""
    K, y_ = np.asarray(K, dtype=float), np.asarray(y_, dtype=float)
    g = np.asarray(group, dtype=np.int64)
    rest = np.setdiff1d(np.arange(len(y_)), g)
    Kgg = K[np.ix_(g, g)]
    if len(rest) == 0:
        return np.full(len(g), float(y_mean)), Kgg * float(y_std) ** 2
    Krr, Kgr = K[np.ix_(rest, rest)], K[np.ix_(g, rest)]
    L = np.linalg.cholesky(Krr)
    A = np.linalg.solve(L, Kgr.T)                       # L^-1 K_rG
    z = np.linalg.solve(L, y_[rest])
    cov = Kgg - A.T.dot(A)
    return A.T.dot(z) * y_std + y_mean, (cov + cov.T) / 2 * float(y_std) ** 2


def brute_loo(K, y_, y_mean=0.0, y_std=1.0):
    """(mean, var_y) of every single point left out in turn."""
    N = len(y_)
    mean, var = np.empty(N), np.empty(N)
    for i in range(N):
        m, c = brute_leave_out(K, y_, [i], y_mean, y_std)
        mean[i], var[i] = m[0], c[0, 0]
    return mean, var


def brute_sequential(K, y_, y_mean=0.0, y_std=1.0):
    """(mean, var_y) of y_k predicted by the model of the rows before it (the prior for k = 0)."""
    N = len(y_)
    mean, var = np.empty(N), np.empty(N)
    for k in range(N):
        m, c = brute_leave_out(K[:k + 1, :k + 1], y_[:k + 1], [k], y_mean, y_std)
        mean[k], var[k] = m[0], c[0, 0]
    return mean, var


def log_density(y, mean, var):
    return -0.5 * (y - mean) ** 2 / var - 0.5 * np.log(2.0 * np.pi * var)


class NumpyLoo:
    """Mixin for ``tests/oracle_device.OracleDevice``: ``loo`` and ``leave_out`` of gpry_amd/_lib.Device in numpy (the
    same refusals and units; not the same bits)."""

    def _loo_factor(self):
        from gpry_amd._lib import GpryHipError
        if self._factor is None:
            raise GpryHipError("the context holds no valid factor")
        return self._factor[1], self._factor[2]

    def loo(self, want=("mean", "var_y", "var_f", "seq_mean", "seq_var_y")):
        V, a = self._loo_factor()
        res = loo(V, a, self.y_, self.alpha, self.y_mean, self.y_std)
        return {k: (res[k] if k in want or k == "device_ms" else None)
                for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y", "device_ms")}

    def leave_out(self, groups):
        from gpry_amd._lib import GpryHipError
        V, a = self._loo_factor()
        try:
            return leave_out(V, a, self.y_, groups, self.y_mean, self.y_std)
        except ValueError as e:
            raise GpryHipError(str(e))
