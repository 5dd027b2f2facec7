"""numpy float64 closed form of the derivative of a GP's posterior mean in theta, the reference of the
``gpry_mean_theta_grad`` tests, the assertions both test files share and a stand-in device.

theta = [log C, log l_1 .. l_d] and, for a model with a white term, log w last; K = C phi(r) + diag(alpha [+ w]),
alpha_ = K^-1 y_, k_i = C phi(r_i) the cross-kernel row of a point, dk_ia = d k_i / d log l_a = C h(r_i) diff_ia^2 with
h = -phi'(r) / r (Matern 1/2: h diff^2 -> 0 at r = 0).  With U = [(alpha + w) o alpha_, (dK / dlog l_a) alpha_ .., w alpha_] and
W = K^-1 U:
    G_0 = y_std k W_0,   G_a = y_std (dk_a alpha_ - k W_a),   G_w = -y_std k W_w
Two formulations: (a) ``grad_explicit`` with the explicit inverse, (b) ``grad_via_V`` through V = L^-1, W = V^T (V U).
``central_differences`` differentiates the numpy mean itself.  Points are in the unit (transformed) coordinates here; the
checks map them through the x-affine.

The tolerance of a device against (b) is test_lml_hessian_gpu.py's rule PER COLUMN j of G (``column_bound``):
    max|G_dev - G_b|_j <= max(10 max|G_a - G_b|_j, 1e-7 max|G_b|_j)
per column because the log C and log w columns are about 1e-3 of the others and a global bound would not test them.

``ThetaGradDevice`` is the stand-in of ``gpry_amd._lib.Device`` for the tests without a GPU (``lml_hessian_model.HessDevice``
with ``mean_theta_grad``).  Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from loo_fit_model import _matrices, problem  # noqa: F401
from lml_hessian_model import HessDevice

W_FLAG = 0x10
Y_MEAN, Y_STD = 0.3, 1.7
X_LO, X_SPAN = -1.5, 2.5

BASE = [(N, d, kid, white) for (N, d) in [(50, 1), (130, 2), (333, 5)] for kid in range(4) for white in (False, True)]
EXTRA = [(300, 17, 2, True), (256, 32, 0, False), (1100, 8, 3, True), (2500, 4, 1, False)]
CASES = BASE + EXTRA
IDS = [f"n{N}_d{d}_k{kid}{'_w' if white else ''}" for N, d, kid, white in CASES]


def cross_terms(Xq_, X_, theta, kid):
    """(k (M, N), dk (M, N, d)): C phi(r) and its derivative in log l_a, C h(r) diff_a^2 (0 at r = 0)."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    C, ls = math.exp(theta[0]), np.exp(theta[1:d + 1])
    D = ((Xq_[:, None, :] - X_[None, :, :]) / ls) ** 2
    r2 = D.sum(axis=2)
    r = np.sqrt(r2)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        if kid == orc.RBF:
            phi = np.exp(-0.5 * r2)
            h = phi
        elif kid == orc.MATERN12:
            phi = np.exp(-r)
            h = np.where(r > 0.0, phi / r, 0.0)
        elif kid == orc.MATERN32:
            t = math.sqrt(3.0) * r
            phi, h = (1.0 + t) * np.exp(-t), 3.0 * np.exp(-t)
        else:
            t = math.sqrt(5.0) * r
            phi, h = (1.0 + t + t * t / 3.0) * np.exp(-t), (5.0 / 3.0) * (1.0 + t) * np.exp(-t)
    return C * phi, C * h[:, :, None] * D


def _rhs(alpha, al, dKs, d, white, theta):
    w = math.exp(theta[d + 1]) if white else 0.0
    cols = [(np.broadcast_to(alpha, al.shape) + w) * al] + [dKs[a].dot(al) for a in range(1, d + 1)]
    if white:
        cols.append(w * al)
    return np.stack(cols, axis=1)


def _assemble(k, dk, al, Wm, d, white, y_std):
    G = np.empty((k.shape[0], Wm.shape[1]))
    G[:, 0] = k.dot(Wm[:, 0])
    for a in range(d):
        G[:, 1 + a] = dk[:, :, a].dot(al) - k.dot(Wm[:, 1 + a])
    if white:
        G[:, d + 1] = -k.dot(Wm[:, d + 1])
    return y_std * G


def grad_explicit(X_, y_, alpha, theta, kid, white, Xq_, y_std=1.0):
    """Formulation (a): explicit inverse."""
    d = X_.shape[1]
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    al = Kinv.dot(y_)
    Wm = Kinv.dot(_rhs(alpha, al, dKs, d, white, theta))
    k, dk = cross_terms(Xq_, X_, theta, kid)
    return _assemble(k, dk, al, Wm, d, white, y_std)


def weights_via_V(X_, y_, alpha, theta, kid, white):
    """(alpha_, W) of formulation (b): V = L^-1, W = V^T (V U)."""
    d = X_.shape[1]
    K, dKs = _matrices(X_, alpha, theta, kid, white)
    V = solve_triangular(cholesky(K, lower=True), np.eye(len(y_)), lower=True)
    al = V.T.dot(V.dot(y_))
    return al, V.T.dot(V.dot(_rhs(alpha, al, dKs, d, white, theta)))


def grad_via_V(X_, y_, alpha, theta, kid, white, Xq_, y_std=1.0):
    """Formulation (b)."""
    al, Wm = weights_via_V(X_, y_, alpha, theta, kid, white)
    k, dk = cross_terms(Xq_, X_, theta, kid)
    return _assemble(k, dk, al, Wm, X_.shape[1], white, y_std)


def mean_numpy(X_, y_, alpha, theta, kid, white, Xq_, y_mean=0.0, y_std=1.0):
    """The unclipped mean at theta, refactorised."""
    d = X_.shape[1]
    theta = np.asarray(theta, dtype=float)
    K, _ = _matrices(X_, alpha, theta, kid, white)
    L = cholesky(K, lower=True)
    al = solve_triangular(L, solve_triangular(L, y_, lower=True), lower=True, trans=1)
    return y_mean + y_std * orc.kernel_matrix(Xq_, theta[:d + 1], kid, Y=X_).dot(al)


def central_differences(X_, y_, alpha, theta, kid, white, Xq_, y_std=1.0, h=1e-4):
    """Central differences of ``mean_numpy`` in every entry of theta (truncation O(h^2))."""
    theta = np.asarray(theta, dtype=float)
    G = np.empty((len(Xq_), len(theta)))
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        G[:, j] = (mean_numpy(X_, y_, alpha, theta + e, kid, white, Xq_, 0.0, y_std)
                   - mean_numpy(X_, y_, alpha, theta - e, kid, white, Xq_, 0.0, y_std)) / (2.0 * h)
    return G


def column_bound(Ga, Gb):
    """The allowed deviation from (b) per column."""
    return np.maximum(10.0 * np.max(np.abs(Ga - Gb), axis=0), 1e-7 * np.max(np.abs(Gb), axis=0))


def column_dev(G, Gb):
    return np.max(np.abs(G - Gb), axis=0)


# ---------------------------------------------------------------------------------------------- the stand-in
class ThetaGradDevice(HessDevice):
    """``HessDevice`` with ``mean_theta_grad`` (formulation (b) at the factorised theta).  The points are evaluated one at a
    time, so that -- as on the device -- a point's bits do not depend on the batch it comes in."""
    n_tg = 0
    logc_sign = 1.0          # the broken variants of the CPU tests turn these
    ls_factor = 1.0

    @property
    def theta_full(self):
        return np.append(self.theta, math.log(self.w)) if self.white else np.array(self.theta, dtype=float)

    def mean_theta_grad(self, X):
        self.n_tg += 1
        assert self._factor is not None, "model not factorised"
        X = np.atleast_2d(np.asarray(X, dtype=float))
        assert X.shape[1] == self.d and len(X) >= 1 and np.all(np.isfinite(X))
        al, Wm = weights_via_V(self.X_, self.y_, self.alpha, self.theta_full, self.kid, self.white)
        G = np.empty((len(X), self.n_theta))
        for i, x_ in enumerate(self._to_unit(X)):
            k, dk = cross_terms(x_[None, :], self.X_, self.theta_full, self.kid)
            G[i] = _assemble(k, dk, al, Wm, self.d, self.white, self.y_std)[0]
        G[:, 0] *= self.logc_sign
        G[:, 1:self.d + 1] *= self.ls_factor
        y = np.array([HessDevice.predict(self, x[None, :])[0] for x in X])
        if getattr(self, "gates", None) is not None:
            y = np.where(self._gate_bits(X) != 0, -np.inf, y)
        return {"y": y, "G": G, "device_ms": 0.0}


# ---------------------------------------------------------------------------------------------- the models and points
def case_index(case):
    return CASES.index(case) if case in CASES else 0


def affine(case):
    """(x_lo, x_span) of the case, None for the half without an x-affine."""
    d = case[1]
    if case_index(case) % 2 == 0:
        return None, None
    return np.full(d, X_LO) - 0.1 * np.arange(d), np.full(d, X_SPAN) + 0.05 * np.arange(d)


def to_raw(case, Xq_):
    lo, span = affine(case)
    return Xq_ if lo is None else lo + span * Xq_


def points(case, X_):
    """26 points in unit coordinates: 8 training rows (0 and 1, which are duplicates, among them), 16 uniform, 2 far outside."""
    N, d = X_.shape
    rng = np.random.default_rng(7 * N + d)
    rows = np.concatenate([[0, 1], rng.choice(np.arange(2, N), 6, replace=False)])
    far = np.stack([np.full(d, 2000.0), np.full(d, -1500.0)])
    return np.concatenate([X_[rows], rng.uniform(0, 1, (16, d)), far])


def load(dev, case, clip_hi=np.inf, theta=None):
    """The case's model on ``dev``, factorised; returns (X_, y_, alpha, theta)."""
    N, d, kid, white = case
    X_, y_, a, th = problem(N, d, seed=N + d, white=white)
    th = th if theta is None else theta
    lo, span = affine(case)
    dev.set_train(X_, y_, a)
    dev.set_theta(kid | W_FLAG if white else kid, th)
    dev.set_affine(lo, span, Y_MEAN, Y_STD, clip_hi)
    assert dev.factorize() == 0
    return X_, y_, a, th


_ref = {}


def reference(case):
    """(Xq_ unit points, G_a, G_b) of the case, computed once and never changed."""
    if case not in _ref:
        N, d, kid, white = case
        X_, y_, a, th = problem(N, d, seed=N + d, white=white)
        Xq_ = points(case, X_)
        Ga = grad_explicit(X_, y_, a, th, kid, white, Xq_, Y_STD)
        Gb = grad_via_V(X_, y_, a, th, kid, white, Xq_, Y_STD)
        for arr in (Xq_, Ga, Gb):
            arr.setflags(write=False)
        _ref[case] = (Xq_, Ga, Gb)
    return _ref[case]


# ---------------------------------------------------------------------------------------------- the assertions
def check_closed_form(dev, case, label=""):
    """G of the device against formulation (b), column by column; returns the worst ratio deviation / bound."""
    N, d, kid, white = case
    load(dev, case)
    Xq_, Ga, Gb = reference(case)
    out = dev.mean_theta_grad(to_raw(case, Xq_))
    G = out["G"]
    p = d + 1 + int(white)
    assert G.shape == (len(Xq_), p) and np.isfinite(G).all()
    dev_j, bound = column_dev(G, Gb), column_bound(Ga, Gb)
    ratio = dev_j / bound
    print(f"mean_theta_grad {label}: worst column ratio {ratio.max():.3f} (column {int(np.argmax(ratio))}), deviation per colmax "
          f"{np.max(dev_j / np.max(np.abs(Gb), axis=0)):.2e}, a-b per colmax "
          f"{np.max(np.max(np.abs(Ga - Gb), axis=0) / np.max(np.abs(Gb), axis=0)):.2e}")
    assert np.all(dev_j <= bound), (dev_j, bound)
    # far outside: k underflows, G is finite (and tiny)
    assert np.all(np.abs(G[-2:]) <= 1e-6 * np.max(np.abs(Gb), axis=0) + bound)
    return float(ratio.max())


def check_value_clip_gates(dev, case):
    """y is predict's one-point answer; a clip or a gate changes y and leaves G as it was."""
    N, d, kid, white = case
    load(dev, case)
    Xq = to_raw(case, reference(case)[0])
    free = dev.mean_theta_grad(Xq)
    one = np.array([dev.predict(x[None, :])[0] for x in Xq])
    assert np.array_equal(free["y"], one)
    clip = float(np.median(free["y"]))
    load(dev, case, clip_hi=clip)
    clipped = dev.mean_theta_grad(Xq)
    assert np.array_equal(clipped["y"], np.minimum(free["y"], clip)) and np.any(free["y"] > clip)
    assert np.array_equal(clipped["y"], np.array([dev.predict(x[None, :])[0] for x in Xq]))
    assert np.array_equal(clipped["G"], free["G"])
    # a trust box that leaves the first half of the points inside nothing: those are gated
    lo_hi = np.stack([Xq.min(axis=0) - 1.0, Xq.max(axis=0) + 1.0], axis=1)
    lo_hi[0, 1] = np.sort(Xq[:, 0])[len(Xq) // 2]
    dev.set_gates(trust_bounds=lo_hi)
    try:
        gated = dev.mean_theta_grad(Xq)
    finally:
        dev.set_gates()
    out = Xq[:, 0] > lo_hi[0, 1]
    assert out.any() and not out.all()
    assert np.all(np.isneginf(gated["y"][out])) and np.array_equal(gated["y"][~out], clipped["y"][~out])
    assert np.isfinite(gated["G"]).all() and np.array_equal(gated["G"], free["G"])
    load(dev, case)
    assert np.array_equal(dev.mean_theta_grad(Xq)["G"], free["G"])


def check_same_bits(dev, case, other):
    """Alone, in a batch, at any position, in split calls, on a second context; a second call repeats the first."""
    load(dev, case)
    Xq = to_raw(case, reference(case)[0])
    whole = dev.mean_theta_grad(Xq)
    again = dev.mean_theta_grad(Xq)
    assert np.array_equal(again["G"], whole["G"]) and np.array_equal(again["y"], whole["y"])
    for i in (0, 9, len(Xq) - 1):
        one = dev.mean_theta_grad(Xq[i:i + 1])
        assert np.array_equal(one["G"][0], whole["G"][i]) and one["y"][0] == whole["y"][i]
    perm = np.random.default_rng(1).permutation(len(Xq))
    shuffled = dev.mean_theta_grad(Xq[perm])
    assert np.array_equal(shuffled["G"], whole["G"][perm]) and np.array_equal(shuffled["y"], whole["y"][perm])
    a, b = dev.mean_theta_grad(Xq[:11]), dev.mean_theta_grad(Xq[11:])
    assert np.array_equal(np.vstack([a["G"], b["G"]]), whole["G"])
    load(other, case)
    o = other.mean_theta_grad(Xq)
    assert np.array_equal(o["G"], whole["G"]) and np.array_equal(o["y"], whole["y"])


def check_against_own_differences(dev, case, h=1e-4):
    """Central differences through set_theta + factorize + predict of the device itself, per column within ten times what
    the numpy central differences miss the numpy closed form by on the same model and step (floor 1e-7 of the column)."""
    N, d, kid, white = case
    X_, y_, a, th = load(dev, case)
    Xq_ = reference(case)[0][:24]                      # (without the far points: nothing to differentiate there)
    Xq = to_raw(case, Xq_)
    G = dev.mean_theta_grad(Xq)["G"]
    fd = np.empty_like(G)
    for j in range(len(th)):
        e = np.zeros(len(th))
        e[j] = h
        vals = []
        for sgn in (1.0, -1.0):
            dev.set_theta(kid | W_FLAG if white else kid, th + sgn * e)
            assert dev.factorize() == 0
            vals.append(dev.predict(Xq))
        fd[:, j] = (vals[0] - vals[1]) / (2.0 * h)
    load(dev, case)
    Gb = grad_via_V(X_, y_, a, th, kid, white, Xq_, Y_STD)
    fd_np = central_differences(X_, y_, a, th, kid, white, Xq_, Y_STD, h)
    colmax = np.max(np.abs(Gb), axis=0)
    bound = np.maximum(10.0 * np.max(np.abs(fd_np - Gb), axis=0), 1e-7 * colmax)
    dev_j = np.max(np.abs(G - fd), axis=0)
    print(f"mean_theta_grad against the device's own differences n{N}_d{d}_k{kid}{'_w' if white else ''}: worst column ratio "
          f"{np.max(dev_j / bound):.3f}, deviation per colmax {np.max(dev_j / colmax):.2e}")
    assert np.all(dev_j <= bound), (dev_j, bound)
    return float(np.max(dev_j / bound))
