"""Truth, yardstick, models and assertions of the theta-box tests: the objective, the factor and the predictions at the
corners of the box a full hyper-parameter fit draws its restarts from (C from 1e-4 to 1e6, every length scale from 1e-3 to
10 box widths, alpha = 1e-4), where cond(K) reaches 1e10 .. 1e13 and the fixed tolerances of the suite are below what
float64 itself delivers.

``truth``      everything in ``np.longdouble`` (``loo_fit_model.factor_extended`` and what follows from it).
``yardstick``  E64, the float64 noise level of ONE model, one number per quantity: the largest deviation from ``truth`` of
               two numpy float64 formulations (the oracle's ``cho_solve`` route and the V-route the device takes), each on the
               training rows as given and under two fixed row permutations -- six samples.
``check_*``    the assertions, written once for any object with the ``Device`` methods they use: every bound has the form
               err <= max(10 E64, floor), both errors taken against ``truth``, the floors the suite's fixed tolerances.
``VRouteDevice``  the float64 V-route as such an object, optionally with every kernel entry multiplied by (1 + s 2^-k).

Test infrastructure only.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gpry_oracle as orc
from loo_fit_model import corr_extended, factor_extended, sqdist_extended

LD = np.longdouble
EXTENDED = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
ALPHA = 1e-4
Y_MEAN, Y_STD = 0.3, 1.7                    # the affine map (None, None, 0.3, 1.7)
SIZES = [(100, 3), (130, 2), (333, 5)]
N_BORDER = 7
FACTOR = 10.0                               # tests/test_lml_hessian_gpu.py: ten times the disagreement of two numpy formulations

# (name, C, l, jittered): l a number or "alternate" (dimensions at 1e-3 and 10 in turn)
THETAS = [("C1e6_l1e-3", 1e6, 1e-3, False), ("C1e6_l10", 1e6, 10.0, False), ("C1e6_l1j", 1e6, 1.0, True),
          ("C1e-4_l10", 1e-4, 10.0, False), ("C1e-4_l1e-3", 1e-4, 1e-3, False), ("C1e2_l3j", 1e2, 3.0, True),
          ("C1e6_aniso", 1e6, "alternate", False)]
MODERATE = 5                                # index of (1e2; 3, jittered)


def theta_of(ti, d):
    name, C, l, jitter = THETAS[ti]
    ls = np.where(np.arange(d) % 2 == 0, 1e-3, 10.0) if l == "alternate" else np.full(d, float(l))
    if jitter:
        ls = ls * 10.0 ** np.random.default_rng(1000 + 10 * ti + d).uniform(-0.3, 0.3, d)
    return np.log(np.append(C, ls))


def data(N, d):
    """X uniform in the unit cube with row 1 a copy of row 0, y_ = standardised sin(3 sum x) + 0.05 noise."""
    rng = np.random.default_rng(100 * N + d)
    X_ = rng.uniform(0, 1, (N, d))
    X_[1] = X_[0]
    y = np.sin(3 * X_.sum(1)) + 0.05 * rng.standard_normal(N)
    return X_, (y - y.mean()) / y.std()


def queries(X_, theta, seed=5):
    """40 points: 30 uniform, 5 on training rows, 5 at l_0 / 5 from a training row along the first axis."""
    N, d = X_.shape
    rng = np.random.default_rng(seed)
    Xq = rng.uniform(0, 1, (40, d))
    Xq[30:35] = X_[[0, 2, N // 3, N // 2, N - 1]]
    Xq[35:40] = X_[[1, 3, N // 4, N // 2 + 1, N - 2]]
    Xq[35:40, 0] += math.exp(theta[1]) / 5.0
    return Xq


GRAD_POINTS = (0, 30, 35)                   # a uniform point, one on a training row, one at l / 5 from a row


def grid_model(C):
    """The exact limit: RBF on the 12 x 12 grid in the unit square with l = 1e-3 -- every off-diagonal entry underflows to 0."""
    g = np.linspace(0.0, 1.0, 12)
    X_ = np.array([[a, b] for a in g for b in g])
    rng = np.random.default_rng(12)
    y = np.sin(3 * X_.sum(1)) + 0.05 * rng.standard_normal(len(X_))
    y_ = (y - y.mean()) / y.std()
    return X_, y_, np.log([C, 1e-3, 1e-3])


def exact_limit(y_, log_C, alpha=ALPHA):
    """(LML, d LML / d log C) of K = (C + alpha) I in extended precision."""
    y = np.asarray(y_, dtype=LD)
    C = np.exp(LD(log_C))
    N, s, yy = len(y), C + LD(alpha), y.dot(y)
    lml = -yy / (2 * s) - LD(N) / 2 * np.log(s) - LD(N) / 2 * np.log(2 * LD(np.pi))
    return lml, C / 2 * (yy / (s * s) - LD(N) / s)


# ------------------------------------------------------------------------------------------------ truth
def _h_extended(r2, kid):
    """h(r) with d k / d log l_j = h D_j and d k / d x_j = -h diff_j / l_j (``corr_and_h``); Matern-1/2: h = 0 at r = 0."""
    if kid == orc.RBF:
        return np.exp(-r2 / 2)
    r = np.sqrt(r2)
    if kid == orc.MATERN12:
        h = np.zeros_like(r)
        nz = r != 0
        h[nz] = np.exp(-r[nz]) / r[nz]
        return h
    t = r * np.sqrt(LD(2 * orc._NU[kid]))
    return 3 * np.exp(-t) if kid == orc.MATERN32 else LD(5) / 3 * (t + 1) * np.exp(-t)


def truth(X_, y_, alpha, theta, kid, Xq=None):
    """K, L, V, alpha_, the LML and its gradient 1/2 sum (alpha alpha^T - K^-1) o dK / d theta_j, and for ``Xq`` the mean, the
    variance C - |V k*|^2 and d k* / d x (transformed units), all in ``np.longdouble``.  ``None`` where a pivot is not positive."""
    f = factor_extended(X_, alpha, theta, kid)
    if f is None:
        return None
    K, L, V = f
    X, y, th = np.asarray(X_, dtype=LD), np.asarray(y_, dtype=LD), np.asarray(theta, dtype=LD)
    N, d = X.shape
    C, ls = np.exp(th[0]), np.exp(th[1:])
    al = V.T.dot(V.dot(y))
    lml = -y.dot(al) / 2 - np.sum(np.log(np.diag(L))) - LD(N) / 2 * np.log(2 * LD(np.pi))
    W = np.outer(al, al) - V.T.dot(V)
    Kc = K.copy()
    Kc[np.diag_indices(N)] = C                                  # d K / d log C: no noise on the diagonal
    Wh = W * (C * _h_extended(sqdist_extended(X, X, ls), kid))
    grad = np.empty(d + 1, dtype=LD)
    grad[0] = np.sum(W * Kc) / 2
    Xs = X / ls
    for j in range(d):
        df = Xs[:, None, j] - Xs[None, :, j]
        grad[1 + j] = np.sum(Wh * (df * df)) / 2
    t = dict(K=K, L=L, V=V, alpha_=al, lml=lml, grad=grad, C=C)
    if Xq is not None:
        Q = np.asarray(Xq, dtype=LD)
        r2 = sqdist_extended(Q, X, ls)
        ks = C * corr_extended(r2, kid)
        U = V.dot(ks.T)
        t["mean"] = ks.dot(al)
        t["var"] = C - np.einsum("ji,ji->i", U, U)
        h = C * _h_extended(r2, kid)
        G = -h[:, :, None] * ((Q[:, None, :] - X[None, :, :]) / ls) / ls
        if kid == orc.MATERN12:
            G = np.where((r2 == 0)[:, :, None], -C / ls, G)     # the r = 0 value of the reference: -C / l
        t["kgrad"] = G                                          # (M, N, d)
    return t


# ------------------------------------------------------------------------------------------------ yardstick
def v_route(X_, y_, alpha, theta, kid, Xq=None, scale=None, scale_q=None):
    """The formulation of the device in numpy float64: V = solve_triangular(L, I), alpha_ = V^T (V y), K^-1 = V^T V.
    ``scale`` / ``scale_q``: factors on the entries of K and of k* (the perturbed stand-in)."""
    theta = np.asarray(theta, dtype=float)
    K, dK = orc.kernel_matrix(X_, theta, kid, eval_gradient=True)
    if scale is not None:
        K = K * scale
    Kn = K.copy()
    Kn[np.diag_indices_from(K)] += alpha
    r = dict(K=Kn)
    try:
        L = cholesky(Kn, lower=True)
    except np.linalg.LinAlgError as e:
        msg = str(e)
        r["info"] = int(msg.split("-th")[0]) if "-th" in msg else 1
        return r
    N = len(y_)
    V = solve_triangular(L, np.eye(N), lower=True)
    al = V.T.dot(V.dot(y_))
    W = np.outer(al, al) - V.T.dot(V)
    r.update(info=0, L=L, V=V, alpha_=al,
             lml=float(-0.5 * y_.dot(al) - np.log(np.diag(L)).sum() - 0.5 * N * math.log(2 * math.pi)),
             grad=np.array([0.5 * np.sum(W * dK[:, :, j]) for j in range(dK.shape[2])]))
    if Xq is not None:
        ks = orc.kernel_matrix(Xq, theta, kid, Y=X_)
        if scale_q is not None:
            ks = ks * scale_q
        U = V.dot(ks.T)
        r["mean"] = ks.dot(al)
        r["var"] = math.exp(theta[0]) - np.einsum("ji,ji->i", U, U)
    return r


def oracle_route(X_, y_, alpha, theta, kid, Xq=None):
    """The oracle's ``cho_solve`` route: ``log_marginal_likelihood`` and ``OracleGPR.predict``."""
    lml, grad = orc.log_marginal_likelihood(X_, y_, alpha, theta, kid, eval_gradient=True)
    r = dict(lml=float(lml), grad=np.asarray(grad), info=int(not np.isfinite(lml)))
    if Xq is not None and r["info"] == 0:
        d = X_.shape[1]
        m = orc.OracleGPR(np.array([[0.0, 1.0]] * d), kernel_id=kid, normalize_X=False, normalize_y=False, clip_factor=None)
        m.X_train_, m.y_train_, m.alpha = X_, y_, alpha
        m.theta, m.newly_appended = np.asarray(theta, dtype=float), 1
        m._update_model()
        mean, std = m.predict(Xq, return_std=True)
        r["mean"], r["var"] = mean, std * std
    return r


def row_orders(N):
    return [np.arange(N)] + [np.random.default_rng(s).permutation(N) for s in (71, 72)]


def yardstick(X_, y_, alpha, theta, kid, Xq, t):
    """E64 per quantity (lml, grad, mean, var: transformed units) and the six samples behind it; ``L``: scipy's float64
    Cholesky against truth; ``kgrad``: the oracle's ``kernel_gradient_x`` against truth at GRAD_POINTS."""
    alpha = np.broadcast_to(alpha, (len(y_),))
    samples = []
    for p in row_orders(len(y_)):
        for route in (oracle_route, v_route):
            r = route(X_[p], y_[p], alpha[p], theta, kid, Xq)
            if r["info"] != 0:
                return None
            samples.append({q: float(np.max(np.abs(np.asarray(r[q], dtype=LD) - t[q]))) for q in ("lml", "grad", "mean", "var")})
    e = {q: max(s[q] for s in samples) for q in samples[0]}
    e["samples"] = samples
    e["L"] = float(np.max(np.abs(v_route(X_, y_, alpha, theta, kid)["L"] - t["L"])))
    e["kgrad"] = max(float(np.max(np.abs(orc.kernel_gradient_x(Xq[i], X_, theta, kid) - t["kgrad"][i]))) for i in GRAD_POINTS)
    return e


_models = {}


def model(N, d, kid, ti):
    """One model of the box with its truth and yardstick, computed once per process."""
    key = (N, d, kid, ti)
    if key not in _models:
        X_, y_ = data(N, d)
        theta = theta_of(ti, d)
        Xq = queries(X_, theta)
        alpha = np.full(N, ALPHA)
        t = truth(X_, y_, alpha, theta, kid, Xq)
        e = None if t is None else yardstick(X_, y_, alpha, theta, kid, Xq, t)
        _models[key] = dict(N=N, d=d, kid=kid, ti=ti, name=f"n{N}_d{d}_k{kid}_{THETAS[ti][0]}", X_=X_, y_=y_, alpha=alpha,
                            theta=theta, Xq=Xq, truth=t, e64=e)
    return _models[key]


def load(dev, m, rows=None, alpha=None):
    n = m["N"] if rows is None else rows
    dev.set_train(m["X_"][:n], m["y_"][:n], (m["alpha"] if alpha is None else alpha)[:n])
    dev.set_theta(m["kid"], m["theta"])
    dev.set_affine(None, None, Y_MEAN, Y_STD)


# ------------------------------------------------------------------------------------------------ the assertions
class Options:
    """Options of the context for the length of a ``with`` block, the defaults put back behind it."""
    DEFAULTS = {"lml_small": 1, "chol_stacked": 2048, "lml_schedule": 0}

    def __init__(self, dev, **opts):
        self.dev, self.opts = dev, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.dev.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.dev.set_option(k, self.DEFAULTS[k])


def objective_paths(dev, N, thetas):
    """Every path that evaluates the objective at a model of N rows: name -> list of (lml, grad, info), one per theta.
    The two single-evaluation paths of the size come first."""
    thetas = np.atleast_2d(thetas)
    out = {}
    out["lml"] = [dev.lml(th, True) for th in thetas]
    second = dict(lml_small=0) if N <= 128 else dict(chol_stacked=0)
    with Options(dev, **second):
        out["lml_" + "_".join(f"{k}{v}" for k, v in second.items())] = [dev.lml(th, True) for th in thetas]
    if N <= 128:
        with Options(dev, lml_small=0, chol_stacked=0):
            out["lml_lml_small0_chol_stacked0"] = [dev.lml(th, True) for th in thetas]
    for name, opts in (("batch_latency", dict(lml_schedule=0)), ("batch_throughput", dict(lml_schedule=1)),
                       ("batch_throughput_lml_small0", dict(lml_schedule=1, lml_small=0))):
        if "lml_small" in opts and N > 128:
            continue
        with Options(dev, **opts):
            l, g, i = dev.lml_batch(thetas, True)
        out[name] = [(float(l[b]), g[b], int(i[b])) for b in range(len(thetas))]
    return out


def report(rows, m, path, **pairs):
    """One line per model, path and quantity: device error, E64, ratio (collected for profiles/theta_box.md)."""
    for q, (err, e64) in pairs.items():
        ratio = err / e64 if e64 > 0 else (0.0 if err == 0 else math.inf)
        print(f"theta_box {m['name']} {path} {q}: err {err:.3e} E64 {e64:.3e} ratio {ratio:.2f}")
        if rows is not None:
            rows.append((m["name"], path, q, err, e64, ratio))


def check_factorises_everywhere(m):
    """LAPACK float64 (both routes, every row order) and long double factorise the model: asserted before the device is asked."""
    assert m["truth"] is not None, m["name"]
    assert m["e64"] is not None, m["name"]


def check_objective(dev, m, rows=None):
    check_factorises_everywhere(m)
    t, e = m["truth"], m["e64"]
    load(dev, m)
    other = theta_of(MODERATE, m["d"])
    paths = objective_paths(dev, m["N"], [m["theta"], other, m["theta"]])
    lml_t, g_t = t["lml"], t["grad"]
    for path, res in paths.items():
        for b in (0, 2):
            lml, grad, info = res[b]
            assert info == 0, (m["name"], path, info)
            assert np.isfinite(lml) and np.isfinite(grad).all(), (m["name"], path)
            el, eg = float(abs(LD(lml) - lml_t)), float(np.max(np.abs(np.asarray(grad, dtype=LD) - g_t)))
            if b == 0:
                report(rows, m, path, lml=(el, e["lml"]), grad=(eg, e["grad"]))
            assert el <= max(FACTOR * e["lml"], 1e-10 * max(1.0, float(abs(lml_t)))), (m["name"], path, el, e["lml"])
            assert eg <= max(FACTOR * e["grad"], 1e-7 * max(1.0, float(np.max(np.abs(g_t))))), (m["name"], path, eg, e["grad"])
        assert res[1][2] == 0, (m["name"], path)
    # the latency batch keeps the bits of the single call
    for b in range(3):
        assert paths["batch_latency"][b][0] == paths["lml"][b][0], (m["name"], b)
        assert np.array_equal(paths["batch_latency"][b][1], paths["lml"][b][1]), (m["name"], b)
    with Options(dev, chol_stacked=0):
        load(dev, m)
        assert dev.factorize() == 0, m["name"]
    load(dev, m)
    assert dev.factorize() == 0, m["name"]


def check_exact_limit(dev, C):
    X_, y_, theta = grid_model(C)
    N = len(y_)
    dev.set_train(X_, y_, np.full(N, ALPHA))
    dev.set_theta(orc.RBF, theta)
    dev.set_affine(None, None, Y_MEAN, Y_STD)
    lml_t, gc_t = exact_limit(y_, theta[0])
    for path, res in objective_paths(dev, N, [theta]).items():
        lml, grad, info = res[0]
        print(f"theta_box exact limit C={C:g} {path}: lml err {float(abs(LD(lml) - lml_t)):.3e} "
              f"log C entry err {float(abs(LD(grad[0]) - gc_t)):.3e} length-scale entries {grad[1:]}")
        assert info == 0, (C, path, info)
        assert abs(LD(lml) - lml_t) <= 1e-10 * max(1.0, float(abs(lml_t))), (C, path)
        assert abs(LD(grad[0]) - gc_t) <= 1e-7 * max(1.0, float(abs(gc_t))), (C, path)
        assert np.all(grad[1:] == 0.0), (C, path, grad)
    assert dev.factorize() == 0


def check_not_positive_definite(dev, N, d, kid):
    """C = 1e6, alpha = 0, row 1 a copy of row 0: (-inf, zero gradient, info > 0) on every path, and the two
    single-evaluation paths of the size report the same column."""
    X_, y_ = data(N, d)
    theta = theta_of(2, d)
    dev.set_train(X_, y_, np.zeros(N))
    dev.set_theta(kid, theta)
    dev.set_affine(None, None, Y_MEAN, Y_STD)
    paths = objective_paths(dev, N, [theta])
    for path, res in paths.items():
        lml, grad, info = res[0]
        print(f"theta_box not positive definite n{N}_d{d}_k{kid} {path}: lml {lml} info {info}")
        assert lml == -np.inf and not np.any(grad) and info > 0, (N, d, kid, path, lml, info)
    single = list(paths)[:2]
    assert paths[single[0]][0][2] == paths[single[1]][0][2], (N, d, kid, single, paths[single[0]][0][2], paths[single[1]][0][2])
    assert dev.factorize() > 0


def resid_L(K, L):
    """|L L^T - K|max / max|K| in long double."""
    K, L = np.asarray(K, dtype=LD), np.asarray(L, dtype=LD)
    return float(np.max(np.abs(L.dot(L.T) - K)) / np.max(np.abs(K)))


def resid_V(L, V):
    """|V L - I|max in long double."""
    L, V = np.asarray(L, dtype=LD), np.asarray(V, dtype=LD)
    return float(np.max(np.abs(V.dot(L) - np.eye(len(L), dtype=LD))))


def resid_alpha(K, a, y_):
    """The backward residual |K a - y|inf / (|K|inf |a|inf + |y|inf) in long double."""
    K, a, y = np.asarray(K, dtype=LD), np.asarray(a, dtype=LD), np.asarray(y_, dtype=LD)
    return float(np.max(np.abs(K.dot(a) - y)) / (np.max(np.sum(np.abs(K), axis=1)) * np.max(np.abs(a)) + np.max(np.abs(y))))


def check_factor(dev, m, rows=None):
    check_factorises_everywhere(m)
    t, e = m["truth"], m["e64"]
    N, C = m["N"], float(t["C"])
    for path, opts in (("factorize", {}), ("factorize_chol_stacked0", dict(chol_stacked=0))):
        with Options(dev, **opts):
            load(dev, m)
            assert dev.factorize() == 0, (m["name"], path)
            L, V, a = dev.get_factor()
            K = dev.kernel_train(add_alpha=True)
        assert all(np.isfinite(x).all() for x in (K, L, V, a)), (m["name"], path)
        assert np.all(np.triu(L, 1) == 0.0) and np.all(np.triu(V, 1) == 0.0), (m["name"], path)
        ek = float(np.max(np.abs(np.asarray(K, dtype=LD) - t["K"])))
        rl, rv, ra = resid_L(K, L), resid_V(L, V), resid_alpha(K, a, m["y_"])
        # yardsticks on the same matrices: solve_triangular on the device's L, the V-route on the device's K
        rv_ref = resid_V(L, solve_triangular(L, np.eye(N), lower=True))
        V64 = solve_triangular(cholesky(K, lower=True), np.eye(N), lower=True)
        ra_ref = resid_alpha(K, V64.T.dot(V64.dot(m["y_"])), m["y_"])
        print(f"theta_box {m['name']} {path}: K err {ek / C:.3e} of C, |L L^T - K| {rl:.3e} of max|K|")
        report(rows, m, path, V=(rv, rv_ref), alpha_=(ra, ra_ref))
        assert ek <= 1e-13 * C, (m["name"], path, ek / C)
        assert rl < 1e-13, (m["name"], path, rl)
        assert rv <= max(FACTOR * rv_ref, 1e-9), (m["name"], path, rv, rv_ref)
        assert ra <= max(FACTOR * ra_ref, N * 2.0 ** -52), (m["name"], path, ra, ra_ref)
    # bordered append: the first N - 7 rows factorised, the last 7 appended
    load(dev, m, rows=N - N_BORDER)
    assert dev.factorize() == 0, m["name"]
    info = dev.append_rows(m["X_"][N - N_BORDER:], m["y_"][N - N_BORDER:], m["alpha"][N - N_BORDER:])
    assert info == 0, (m["name"], info)
    L2 = dev.get_factor(want_V=False, want_alpha=False)[0]
    el = float(np.max(np.abs(np.asarray(L2, dtype=LD) - t["L"])))
    report(rows, m, "append_rows", L=(el, e["L"]))
    assert el <= max(FACTOR * e["L"], 1e-10 * float(np.max(np.abs(t["L"])))), (m["name"], el, e["L"])


def check_predictions(dev, m, rows=None):
    check_factorises_everywhere(m)
    t, e = m["truth"], m["e64"]
    Xq, C, kid = m["Xq"], float(t["C"]), m["kid"]
    load(dev, m)
    assert dev.factorize() == 0, m["name"]
    mean_t = Y_MEAN + Y_STD * t["mean"]
    var_t = t["var"] * (Y_STD * Y_STD)
    e_mean, e_var = Y_STD * e["mean"], Y_STD * Y_STD * e["var"]
    floor_mean = 1e-8 * max(1.0, float(np.max(np.abs(Y_MEAN + Y_STD * m["y_"]))))
    floor_var = 1e-9 * C * Y_STD * Y_STD
    got = {"predict_3": (dev.predict(Xq[:3]), None, slice(0, 3))}
    mean, std = dev.predict(Xq, return_std=True)
    got["predict_40"] = (mean, std, slice(None))
    out = dev.sweep_logexp(Xq, orc.auto_zeta(m["d"]), float(np.max(Y_MEAN + Y_STD * m["y_"])), 1e-2 * Y_STD, want=("y", "sigma"))
    form = dev.sweep_info()["panel_form"]
    got["sweep_logexp"] = (out["y"], out["sigma"], slice(None))
    print(f"theta_box {m['name']} sweep_logexp: panel form {form}")
    for path, (mean, std, sl) in got.items():
        assert np.isfinite(mean).all(), (m["name"], path)
        em = float(np.max(np.abs(np.asarray(mean, dtype=LD) - mean_t[sl])))
        pairs = dict(mean=(em, e_mean))
        if std is not None:
            assert np.isfinite(std).all(), (m["name"], path)
            ev = float(np.max(np.abs(np.asarray(std, dtype=LD) ** 2 - var_t[sl])))
            pairs["var"] = (ev, e_var)
        report(rows, m, path + (f"[{form}]" if path == "sweep_logexp" else ""), **pairs)
        assert em <= max(FACTOR * e_mean, floor_mean), (m["name"], path, em, e_mean)
        if std is not None:
            assert ev <= max(FACTOR * e_var, floor_var), (m["name"], path, ev, e_var)
    for i in GRAD_POINTS:
        G = dev.predict_grad(Xq[i], want_kinv=True, want_kgrad=True)[2]
        Gt = t["kgrad"][i]
        assert np.isfinite(G).all(), (m["name"], i)                 # Matern-1/2 on a training row: the r = 0 value, never NaN
        eg = float(np.max(np.abs(np.asarray(G, dtype=LD) - Gt)))
        big = float(np.max(np.abs(Gt)))
        if i == GRAD_POINTS[1] and kid == orc.MATERN12:
            j = int(np.argmin(np.sum((m["X_"] - Xq[i]) ** 2, axis=1)))
            assert np.array_equal(G[j], -C / np.exp(m["theta"][1:])) or eg <= 1e-10 * big, (m["name"], G[j])
        report(rows, m, f"predict_grad[{i}]", kgrad=(eg, e["kgrad"]))
        assert eg <= max(FACTOR * e["kgrad"], 1e-10 * big), (m["name"], i, eg, e["kgrad"], big)


# ------------------------------------------------------------------------------------------------ the stand-in
class VRouteDevice:
    """The float64 V-route behind the ``Device`` methods the assertions use.  ``k``: every kernel entry (training matrix and
    cross kernel) is multiplied by (1 + s 2^-k), s = +-1 from a fixed seed (symmetric in the training matrix)."""

    def __init__(self, k=None, seed=9):
        self.k, self.seed = k, seed
        self.options = dict(Options.DEFAULTS)
        self._f = None

    def set_option(self, key, value):
        self.options[key] = int(value)

    def set_train(self, X_, y_, alpha):
        self.X_, self.y_ = np.array(X_, dtype=float), np.array(y_, dtype=float)
        self.N, self.d = self.X_.shape
        self.alpha = np.array(np.broadcast_to(alpha, (self.N,)), dtype=float)
        self._f = None

    def set_theta(self, kernel_id, theta):
        self.kid, self.theta = int(kernel_id), np.array(theta, dtype=float)
        self._f = None

    def set_affine(self, x_lo=None, x_span=None, y_mean=0.0, y_std=1.0, clip_hi=np.inf):
        assert x_lo is None and x_span is None
        self.y_mean, self.y_std = float(y_mean), float(y_std)

    def _signs(self, rows, cols, symmetric):
        if self.k is None:
            return None
        s = np.random.default_rng(self.seed).choice([-1.0, 1.0], (rows, cols))
        if symmetric:
            s = np.tril(s) + np.tril(s, -1).T
        return 1.0 + s * 2.0 ** -self.k

    def _run(self, theta, Xq=None):
        return v_route(self.X_, self.y_, self.alpha, theta, self.kid, Xq, self._signs(self.N, self.N, True),
                       None if Xq is None else self._signs(len(Xq), self.N, False))

    def lml(self, theta, eval_gradient=False):
        r = self._run(theta)
        if r["info"] != 0:
            return (-np.inf, np.zeros(self.d + 1), r["info"]) if eval_gradient else (-np.inf, r["info"])
        return (r["lml"], r["grad"], 0) if eval_gradient else (r["lml"], 0)

    def lml_batch(self, thetas, eval_gradient=True):
        res = [self.lml(th, True) for th in np.atleast_2d(thetas)]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res], dtype=np.int32)

    def factorize(self):
        self._f = self._run(self.theta)
        return self._f["info"]

    def kernel_train(self, add_alpha=False):
        K = self._run(self.theta)["K"]
        if not add_alpha:
            K[np.diag_indices_from(K)] -= self.alpha
        return K

    def get_factor(self, want_L=True, want_V=True, want_alpha=True):
        f = self._f
        return (f["L"].copy() if want_L else None, f["V"].copy() if want_V else None, f["alpha_"].copy() if want_alpha else None)

    def append_rows(self, Xnew_, ynew_, alphanew):
        k = len(np.atleast_1d(ynew_))
        self.set_train(np.vstack([self.X_, np.atleast_2d(Xnew_)]), np.append(self.y_, ynew_),
                       np.append(self.alpha, np.broadcast_to(alphanew, (k,))))
        return self.factorize()

    def predict(self, X, return_std=False, mask=None):
        r = self._run(self.theta, np.atleast_2d(X))
        mean = self.y_mean + self.y_std * r["mean"]
        return (mean, self.y_std * np.sqrt(np.maximum(r["var"], 0.0))) if return_std else mean

    def sweep_logexp(self, X, zeta, baseline, sigma_n, mask=None, M=None, want=("y", "sigma", "acq")):
        y, s = self.predict(X, return_std=True)
        return {"y": y, "sigma": s, "acq": None, "n_nan": 0}

    def sweep_info(self):
        return {"panel_form": "none"}

    def predict_grad(self, x, want_kinv=True, want_kgrad=False, want_mean=True):
        G = orc.kernel_gradient_x(np.asarray(x, dtype=float), self.X_, self.theta, self.kid)
        if self.k is not None:
            G = G * self._signs(1, self.N, False)[0][:, None]
        return (None, None, G) if want_kgrad else (None, None)
