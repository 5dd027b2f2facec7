"""numpy restatement of gpry_amd/csrc/svm_fit.hip (``gpry_svm_fit``): the C-SVC dual of two classes with the RBF kernel,
solved by sequential minimal optimisation with libsvm's second-order working-set selection, its two-variable update and
its ``calculate_rho`` (svm.cpp: Solver::select_working_set, Solver::Solve, Solver::calculate_rho), without shrinking.

    minimise 1/2 a^T Q a - sum a,   0 <= a_t <= C,   sum y_t a_t = 0,   Q_ts = y_t y_s exp(-gamma |x_t - x_s|^2)

This file is the written-down order of operations of the kernel:

* ``i`` = argmax of ``-y_t G_t`` over I_up, ``j`` = argmin of ``-b^2 / a`` over the t of I_low with ``b = G_max + y_t G_t > 0``,
  ``a = 2 - 2 k(x_i, x_t)`` (``tau = 1e-12`` for a non-positive one); ties in both go to the SMALLEST index;
* stop when ``G_max - G_min < eps``;
* before convergence is declared G is recomputed from alpha -- per point the rows with alpha > 0 in ascending index
  order -- and the test repeated on it; a failure goes on iterating from the recomputed gradient;
* ``r^2`` is the sum of the squared coordinate differences in coordinate order.

The device fuses multiply and add (``fma``) where numpy rounds twice, and its exponential is the library's own routine:
the two agree to rounding, not bit for bit.  ``NumpySvmFit`` gives a numpy device ``svm_fit``; ``bounds`` are the derived
tolerances that the tests of both sides use; ``labelled_set`` makes their training sets.
"""
import numpy as np

TAU = 1e-12
MAX_N = 8192
MAX_DIM = 32


def kernel_row(X, s, gamma):
    """k(x_s, x_t) for every t: r^2 summed in coordinate order."""
    r2 = np.zeros(len(X))
    for k in range(X.shape[1]):
        df = X[:, k] - X[s, k]
        r2 = df * df + r2
    return np.exp(-(gamma * r2))


def gradient(X, y, alpha, gamma):
    """G = Q alpha - e, the rows with alpha > 0 added in ascending index order."""
    acc = np.zeros(len(X))
    for s in np.flatnonzero(alpha > 0.0):
        acc = (y[s] * alpha[s]) * kernel_row(X, s, gamma) + acc
    return y * acc - 1.0


def _first_argmax(v, member):
    """Smallest index among the members with the largest value (-1: no member)."""
    idx = np.flatnonzero(member)
    if not len(idx):
        return -1
    return int(idx[np.argmax(v[idx])])          # np.argmax returns the first of equal maxima


def select(X, y, alpha, G, C, gamma):
    """(i, j, G_max, G_min, k_i): the working set of libsvm's WSS 2 with the smallest-index tie rule."""
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0.0))
    low = ((y > 0) & (alpha > 0.0)) | ((y < 0) & (alpha < C))
    i = _first_argmax(-y * G, up)
    if i < 0 or not low.any():
        return i, -1, np.nan, np.nan, None
    gmax = float(-y[i] * G[i])
    ki = kernel_row(X, i, gamma)
    yg = y * G
    gmin = -float(np.max(yg[low]))
    b = gmax + yg
    qd = 2.0 - 2.0 * ki
    qd = np.where(qd > 0.0, qd, TAU)
    j = _first_argmax((b * b) / qd, low & (b > 0.0))
    return i, j, gmax, gmin, ki


def step(yi, yj, Gi, Gj, ai, aj, kij, C):
    """libsvm's two-variable update (Solver::Solve) for equal bounds C: the new (alpha_i, alpha_j)."""
    Qij = yi * yj * kij
    if yi != yj:
        quad = 2.0 + 2.0 * Qij
        if not quad > 0.0:
            quad = TAU
        delta, diff = (-Gi - Gj) / quad, ai - aj
        ai, aj = ai + delta, aj + delta
        if diff > 0.0:
            if aj < 0.0:
                aj, ai = 0.0, diff
        elif ai < 0.0:
            ai, aj = 0.0, -diff
        if diff > 0.0:
            if ai > C:
                ai, aj = C, C - diff
        elif aj > C:
            aj, ai = C, C + diff
    else:
        quad = 2.0 - 2.0 * Qij
        if not quad > 0.0:
            quad = TAU
        delta, total = (Gi - Gj) / quad, ai + aj
        ai, aj = ai - delta, aj + delta
        if total > C:
            if ai > C:
                ai, aj = C, total - C
        elif aj < 0.0:
            aj, ai = 0.0, total
        if total > C:
            if aj > C:
                aj, ai = C, total - C
        elif ai < 0.0:
            ai, aj = 0.0, total
    return ai, aj


def rho_of(y, alpha, G, C):
    """libsvm's calculate_rho."""
    yg = y * G
    upper, lower = alpha >= C, alpha <= 0.0
    free = ~upper & ~lower
    if free.any():
        return float(np.sum(yg[free]) / np.count_nonzero(free))
    ub_set = (upper & (y < 0)) | (lower & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & (y < 0))
    ub = np.min(yg[ub_set]) if ub_set.any() else np.inf
    lb = np.max(yg[lb_set]) if lb_set.any() else -np.inf
    return float((ub + lb) / 2.0)


def check_args(X, finite, C, gamma, eps, max_iter):
    X = np.asarray(X, dtype=float)
    finite = np.asarray(finite).astype(bool)
    if X.ndim != 2 or len(finite) != len(X):
        raise ValueError("svm_fit: X must be (N, d) and finite (N,)")
    N, d = X.shape
    if N < 2 or N > MAX_N:
        raise RuntimeError(f"gpry_svm_fit: N = {N}, need 2 <= N <= {MAX_N}")
    if d < 1 or d > MAX_DIM:
        raise RuntimeError(f"gpry_svm_fit: d = {d}, need 1 <= d <= {MAX_DIM}")
    if not all(np.isfinite(v) and v > 0 for v in (C, gamma, eps)):
        raise RuntimeError("gpry_svm_fit: C, gamma and eps must be positive and finite")
    if finite.all() or not finite.any():
        raise RuntimeError("gpry_svm_fit: the labels hold one class only")
    if not np.isfinite(X).all():
        raise RuntimeError("gpry_svm_fit: X holds a non-finite value")
    return X, finite, (100 * N + 10000 if max_iter is None else int(max_iter))


def svm_fit(X, finite, C, gamma, eps=1e-3, max_iter=None):
    """The outputs of ``Device.svm_fit``: alpha, rho, objective, violation, n_iter, status, device_ms."""
    X, finite, max_iter = check_args(X, finite, C, gamma, eps, max_iter)
    C, gamma, eps = float(C), float(gamma), float(eps)
    y = np.where(finite, 1.0, -1.0)
    alpha, G = np.zeros(len(X)), np.full(len(X), -1.0)
    n_iter, status, fresh = 0, 1, False
    gmax = gmin = 0.0
    while True:
        i, j, gmax, gmin, ki = select(X, y, alpha, G, C, gamma)
        if i < 0 or j < 0 or not gmax - gmin >= eps:
            if fresh:
                status = 0
                break
            G, fresh = gradient(X, y, alpha, gamma), True
            continue
        if n_iter >= max_iter:
            break
        ai, aj = step(y[i], y[j], G[i], G[j], alpha[i], alpha[j], ki[j], C)
        ci, cj = y[i] * (ai - alpha[i]), y[j] * (aj - alpha[j])
        kj = kernel_row(X, j, gamma)
        G = (y * kj) * cj + ((y * ki) * ci + G)
        alpha[i], alpha[j] = ai, aj
        n_iter, fresh = n_iter + 1, False
    return dict(alpha=alpha, rho=rho_of(y, alpha, G, C), objective=float(0.5 * np.sum(alpha * (G - 1.0))),
                violation=float(gmax - gmin), n_iter=n_iter, status=status, device_ms=0.0)


class NumpySvmFit:
    """Mix-in that gives a numpy device the call ``svm_fit``."""

    def svm_fit(self, X, finite, C, gamma, eps=1e-3, max_iter=None):
        return svm_fit(X, finite, C, gamma, eps=eps, max_iter=max_iter)


# ---- what the tests of both sides share -----------------------------------------------------------------------------
def kernel_matrix(A, B, gamma):
    r2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A.dot(B.T), 0.0)
    return np.exp(-gamma * r2)


def decision(Xtest, X, y, alpha, rho, gamma, chunk=1024):
    sv = np.flatnonzero(alpha > 0.0)
    coef = y[sv] * alpha[sv]
    out = np.empty(len(Xtest))
    for s in range(0, len(Xtest), chunk):
        out[s:s + chunk] = kernel_matrix(Xtest[s:s + chunk], X[sv], gamma).dot(coef) - rho
    return out


def host_checks(X, finite, alpha, gamma, C):
    """From alpha alone, in numpy: G = Q alpha - e, the two ends of the stop test, the objective and sum y alpha."""
    y = np.where(finite, 1.0, -1.0)
    sv = np.flatnonzero(alpha > 0.0)
    G = y * kernel_matrix(X, X[sv], gamma).dot(y[sv] * alpha[sv]) - 1.0
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0.0))
    low = ((y > 0) & (alpha > 0.0)) | ((y < 0) & (alpha < C))
    gmax = np.max((-y * G)[up]) if up.any() else -np.inf
    gmin = np.min((-y * G)[low]) if low.any() else np.inf
    return dict(G=G, violation=float(gmax - gmin), objective=float(0.5 * np.sum(alpha * (G - 1.0))),
                sum_y_alpha=float(np.sum(y * alpha)), n_sv=len(sv))


def bounds(alpha, alpha_ref, eps, d, n_iter):
    """The derived tolerances (S = sum alpha + sum alpha_ref): objective gap eps S, decision difference
    B = 4 sqrt(2 eps S) + 2 eps, and the rounding of the host's recomputation: (n_SV + d + 10) 2^-53 sum alpha per entry
    of G, 2 n_iter 2^-53 max alpha for the equality constraint."""
    S = float(np.sum(alpha) + np.sum(alpha_ref))
    u = 2.0 ** -53
    n_sv = int(np.count_nonzero(alpha > 0.0))
    return dict(S=S, objective=eps * S, decision=4.0 * np.sqrt(2.0 * eps * S) + 2.0 * eps,
                grad_round=(n_sv + d + 10) * u * float(np.sum(alpha)),
                equality=2.0 * max(n_iter, 1) * u * float(np.max(alpha)))


def labelled_set(N, d, seed, separable=True):
    """Half uniform in the unit cube, half around a Gaussian mode, labelled by a threshold on the Gaussian log-density
    (separable) or by that threshold on a noisy copy of it with a tenth of the labels flipped (overlapping classes: some
    alphas end at C)."""
    rng = np.random.default_rng(seed)
    n_u = N // 2
    centre, width = np.full(d, 0.5), 0.12
    X = np.concatenate([rng.uniform(0.0, 1.0, (n_u, d)), centre + width * rng.standard_normal((N - n_u, d))])
    X = X[rng.permutation(N)]
    logp = -0.5 * np.sum(((X - centre) / width) ** 2, axis=1)
    thr = -0.5 * (2.0 + 1.5 * np.sqrt(d)) ** 2 * 0.5
    score = logp if separable else logp + 0.35 * abs(thr) * rng.standard_normal(N)
    finite = score > thr
    if not separable:
        finite ^= rng.uniform(size=N) < 0.1
    if finite.all() or not finite.any():        # tiny sets: make sure both classes occur
        order = np.argsort(logp)
        finite = np.zeros(N, dtype=bool)
        finite[order[N // 2:]] = True
    return X, finite


def probe_points(X, M, seed):
    """M points to compare decision values at: half uniform in the bounding box of the training set, half scattered
    around training rows (a tenth of the box's size), so that tiny sets are probed where their decision function lives."""
    rng = np.random.default_rng(seed)
    lo, hi = X.min(axis=0), X.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    near = X[rng.integers(0, len(X), M - M // 2)] + 0.1 * span * rng.standard_normal((M - M // 2, X.shape[1]))
    return np.concatenate([lo + span * rng.uniform(0.0, 1.0, (M // 2, X.shape[1])), near])
