"""Step-by-step host reference of the device samplers' walks (gpry_amd/csrc/nested.hip, mcmc.hip), the tables of cases
the walk tests run (tests/test_sampler_walk_cpu.py, tests/test_sampler_walk_gpu.py) and the models behind them.

``traced_generation``: the algorithm of ``ns_philox.NumpyNestedDevice.ns_generation`` (and, with ``labels`` / ``cum_p``,
of ``ns_cluster.ClusteredNumpyDevice`` / ``ns_volumes.VolumesNumpyDevice``: drawn cluster, drawn start, then the walk)
which keeps, per chain and step r = 0 .. R, what a comparison with the kernel needs:

- ``U[r]``, ``X[r]``, ``y[r]``: the state after r steps (unit-cube and raw coordinates), ``ncalls[r]``: the evaluations so far
  -- so that one run of R steps is the reference of ``ns_generation(..., num_repeats=r)`` for every r <= R;
- ``margin_y[r]``, ``margin_g[r]``: the smallest distance of any decision of the walk so far from flipping.  margin_y:
  |y - L*| / (1 + |L*|) of every evaluated try (on a plateau, L* = clip_hi, no try is ever accepted and y is the clip on
  both sides only where the unclipped mean exceeds it: there |mean - clip_hi| / (1 + |clip_hi|)); a gated try (-inf) has
  none (the gates are compared with the host masks elsewhere: tests/tools/fuzz_gates.py).  margin_g: the distance of
  every tried u from the faces 0 and 1, and |t| / max(|lt|, |rt|) of every failed shrinkage try (the sign of t picks the end
  that moves; t = lt + w (rt - lt) carries the rounding of the bracket's larger end, and a walk whose tries all fail
  draws its bracket in to 1e-20 around the start: the distance that counts is relative to the bracket);
- ``stepout[c]``: the largest number of whole widths a chain stepped out on one side of any step (32 = the cap).

The direction is ``v = tril(W) z / |z|``: the kernel sums k <= t only, the contract of ``ns_generation`` is a lower
triangular W (what ``nested.whitening`` / ``cholesky_ridged`` deliver).

Arithmetic.  ``dtype=np.longdouble`` runs the same walk (same draws; the likelihood still in float64) in extended
precision.  The largest |U_float64 - U_longdouble| over the chains x steps the margins keep, over the whole table of
NESTED_CASES, is the arithmetic noise floor of the restatement: eps0 = 2.33e-15 measured (x86 80-bit long double, R = 8; a few
ulp of the unit cube per step times the 33 widths a capped step-out is away from its start), rounded up to EPS0 = 2.5e-15
below; the CPU file measures it again on every run and asserts it stays below EPS0.  The GPU test allows POS_TOL =
100 x EPS0 = 2.5e-13: two orders for what the kernel does differently (FMA contraction of lo + u span and of the direction's
sums, the device's log / cos / sin).  A wrong bracket or direction moves a point by a width of W, > 1e-6 in the unit cube
for the narrowest W of the table (asserted in the CPU file: POS_TOL < 1e-6 x the smallest diagonal entry of any W).

Which chains are compared: those with margin_y > Y_MARGIN = 1e-9 and margin_g > G_MARGIN = 100 x EPS0 up to that step;
the others are left out from that step on and counted.  At most 25 % of a case's chains and 5 % of the table's may be
left out by the last step (LEFT_OUT_CASE, LEFT_OUT_TABLE)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ns_philox import (DRAW_OFFSET, DRAW_SHRINK, PHASE_START, PHASE_STEP, SHRINK_MAX, STEP_OUT_MAX,  # noqa: E402
                       philox, prior_points)
from ns_volumes import drawn_clusters  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import gpry_oracle as orc  # noqa: E402

EPS0 = 2.5e-15
POS_TOL = 100 * EPS0
Y_MARGIN = 1e-9
G_MARGIN = 100 * EPS0
LEFT_OUT_CASE, LEFT_OUT_TABLE = 0.25, 0.05
MEAN_TOL = 1e-7                 # tests/tools/fuzz_parity.py: the mean within 1e-7 of max(1, max |y_train|)
R_STEPS, N_CHAINS = 8, 64

KERNEL_SPEC = {0: "RBF", 1: {"Matern": {"nu": 0.5}}, 2: {"Matern": {"nu": 1.5}}, 3: {"Matern": {"nu": 2.5}}}


def dp_bucket(d):
    """The DP template argument the sampler kernels are dispatched with."""
    return 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def nsplit(N):
    """The slices of the one-point path: clamp(N / 1024, 1, 8)."""
    return min(max(N // 1024, 1), 8)


class Trace:
    def __init__(self, k, d, R):
        self.U, self.X = np.empty((R + 1, k, d)), np.empty((R + 1, k, d))
        self.y = np.empty((R + 1, k))
        self.ncalls = np.zeros((R + 1, k), np.int64)
        self.margin_y, self.margin_g = np.full((R + 1, k), np.inf), np.full((R + 1, k), np.inf)
        self.stepout = np.zeros(k, np.int64)
        self.gated = np.zeros(k, np.int64)          # evaluated tries the gates rejected
        self.start = np.zeros(k, np.int64)
        self.cluster = np.zeros(k, np.int64)

    def keep(self, r):
        """The chains whose decisions up to step r all lie outside the margins."""
        return (self.margin_y[r] > Y_MARGIN) & (self.margin_g[r] > G_MARGIN)

    def take(self, sel, other):
        for name in ("U", "X", "y", "ncalls", "margin_y", "margin_g"):
            getattr(self, name)[:, sel] = getattr(other, name)[:, sel]
        for name in ("stepout", "gated", "start"):
            getattr(self, name)[sel] = getattr(other, name)[sel]


def _walk(mean, clip_hi, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, R, dtype, shift):
    """The unclustered generation.  ``mean(X) -> (m,)``: the unclipped mean, -inf where the gates reject; the likelihood
    is min(mean + shift (1 + |L*|), clip_hi)."""
    ft = dtype
    lo64, hi64 = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    lo, hi = lo64.astype(ft), hi64.astype(ft)
    span = hi - lo
    n, d = X_surv.shape
    tr = Trace(k, d, R)
    c = np.arange(k)
    us, _ = philox(seed, PHASE_START, 0, generation, c, 0)
    j = np.minimum((us * n).astype(np.int64), n - 1)
    tr.start[:] = j
    x = np.asarray(X_surv, dtype=float)[j].astype(ft)
    y = np.asarray(y_surv, dtype=float)[j].copy()
    u = (x - lo) / span
    cnt = np.zeros(k, dtype=np.int64)
    my, mg = np.full(k, np.inf), np.full(k, np.inf)
    Wl = np.tril(np.asarray(W, dtype=float)).astype(ft)
    plateau = lstar >= clip_hi
    yscale = 1.0 + abs(lstar)

    def attempt(t, v, act):
        """(accepted, y, u, x) of the points u + t v of the chains in `act`; updates the counts and the margins."""
        ut = u + t[:, None] * v
        xt = lo + ut * span
        inside = act & np.all((ut >= 0) & (ut <= 1) & (xt >= lo) & (xt <= hi), axis=1)
        face = np.min(np.minimum(np.abs(ut), np.abs(ut - 1)), axis=1).astype(float)
        mg[act] = np.minimum(mg[act], face[act])
        yt = np.full(k, -np.inf)
        if inside.any():
            m = np.asarray(mean(np.ascontiguousarray(xt[inside].astype(float))), dtype=float)
            with np.errstate(invalid="ignore"):
                m = m + shift * yscale
            yt[inside] = np.minimum(m, clip_hi)
            cnt[inside] += 1
            with np.errstate(invalid="ignore"):
                dist = np.abs(m - clip_hi) / (1.0 + abs(clip_hi)) if plateau else np.abs(yt[inside] - lstar) / yscale
            dist = np.where(np.isneginf(m), np.inf, dist)
            tr.gated[inside] += np.isneginf(m)
            my[inside] = np.minimum(my[inside], dist)
        return inside & (yt > lstar), yt, ut, xt

    def record(r):
        tr.U[r], tr.X[r], tr.y[r], tr.ncalls[r] = u.astype(float), x.astype(float), y, cnt
        tr.margin_y[r], tr.margin_g[r] = my, mg

    record(0)
    h = (d + 1) // 2
    two_pi = 2 * np.pi if ft is np.float64 else 8 * np.arctan(ft(1))
    for s in range(R):
        ua, ub = philox(seed, PHASE_STEP, np.arange(h)[None, :], generation, c[:, None], s)
        ua, ub = ua.astype(ft), ub.astype(ft)
        rad, ang = np.sqrt(-2.0 * np.log(1.0 - ua)), two_pi * ub
        z = np.empty((k, 2 * h), dtype=ft)
        z[:, 0::2], z[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
        z = z[:, :d]
        v = z @ Wl.T / np.linalg.norm(z, axis=1)[:, None]
        r, _ = philox(seed, PHASE_STEP, DRAW_OFFSET, generation, c, s)
        lt, rt = (-r).astype(ft), (1.0 - r).astype(ft)
        for side in (-1, 1):
            act = np.ones(k, bool)
            nout = np.zeros(k, np.int64)
            for _ in range(STEP_OUT_MAX):
                ok = attempt(lt if side < 0 else rt, v, act)[0]
                if side < 0:
                    lt = np.where(ok, lt - 1, lt)
                else:
                    rt = np.where(ok, rt + 1, rt)
                nout += ok
                act = ok
                if not act.any():
                    break
            tr.stepout = np.maximum(tr.stepout, nout)
        todo = np.ones(k, bool)
        for q in range(SHRINK_MAX):
            w, _ = philox(seed, PHASE_STEP, DRAW_SHRINK + q, generation, c, s)
            t = lt + w.astype(ft) * (rt - lt)
            ok, yt, ut, xt = attempt(t, v, todo)
            u[ok], x[ok], y[ok] = ut[ok], xt[ok], yt[ok]
            miss = todo & ~ok
            rel = (np.abs(t) / np.maximum(np.abs(lt), np.abs(rt))).astype(float)
            mg[miss] = np.minimum(mg[miss], rel[miss])
            lt = np.where(miss & (t < 0), t, lt)
            rt = np.where(miss & (t >= 0), t, rt)
            todo = miss
            if not todo.any():
                break
        record(s + 1)
    return tr


def traced_generation(mean, clip_hi, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, R, labels=None, cum_p=None,
                      dtype=np.float64, shift=0.0):
    """The trace (see the module's docstring) of ``ns_generation(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k,
    r, labels=, cum_p=)`` for r = 0 .. R."""
    args = (seed, generation, k, R, dtype, shift)
    X_surv, y_surv = np.asarray(X_surv, dtype=float), np.asarray(y_surv, dtype=float)
    if labels is None:
        return _walk(mean, clip_hi, lo, hi, X_surv, y_surv, lstar, W, *args)
    W, labels = np.asarray(W, dtype=float), np.asarray(labels)
    tr = Trace(k, X_surv.shape[1], R)
    if cum_p is None:
        us, _ = philox(seed, PHASE_START, 0, generation, np.arange(k), 0)
        tr.cluster[:] = labels[np.minimum((us * len(X_surv)).astype(np.int64), len(X_surv) - 1)]
        for q in np.unique(tr.cluster):
            tr.take(tr.cluster == q, _walk(mean, clip_hi, lo, hi, X_surv, y_surv, lstar, W[q], *args))
        return tr
    tr.cluster[:] = drawn_clusters(seed, generation, k, cum_p)
    for q in np.unique(tr.cluster):
        mem = np.flatnonzero(labels == q)
        sub = _walk(mean, clip_hi, lo, hi, X_surv[mem], y_surv[mem], lstar, W[q], *args)
        sub.start = mem[sub.start]
        tr.take(tr.cluster == q, sub)
    return tr


# ---- models ---------------------------------------------------------------------------------------------------------
def gauss_ll(d, s=0.5, mu=0.3):
    return lambda X: -0.5 * np.sum((np.atleast_2d(X) - mu) ** 2, axis=1) / s ** 2


def training(ll, d, N, seed, width=4.0, spread=1.0):
    """Half uniform on the box [-width, width]^d, half around the mode (tests/test_nested_gpu.py: _training)."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-width, width, (N // 2, d)),
                        np.clip(rng.normal(0.0, spread, (N - N // 2, d)), -width, width)])
    return np.array([[-width, width]] * d), X, ll(X)


def mirror(bounds, kid, theta, affine=True, normalize_y=True, device=None, **kw):
    """The drop-in regressor with fixed hyper-parameters; ``device``: a test double for runs without a GPU."""
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import clone
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    kw.setdefault("account_for_inf", None)
    gpr = GaussianProcessRegressor(kernel=KERNEL_SPEC[kid], bounds=bounds,
                                   preprocessing_X=Normalize_bounds(bounds) if affine else None,
                                   preprocessing_y=Normalize_y() if normalize_y else None, **kw)
    k = clone(gpr.kernel)
    k.theta = np.asarray(theta, dtype=float)
    gpr.kernel_, gpr._fitted = k, True
    if device is not None:
        gpr._dev = device
    return gpr


def oracle_of(bounds, kid, theta, X, y, affine=True, normalize_y=True, **kw):
    """The float64 numpy model of the same data and hyper-parameters (oracle.gpry_oracle.OracleGPR)."""
    ref = orc.OracleGPR(bounds, kernel_id=kid, normalize_X=affine, normalize_y=normalize_y, **kw)
    ref.theta = np.asarray(theta, dtype=float).copy()
    ref.fitted = True
    ref.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    return ref


class Model:
    """The data and hyper-parameters of a case; ``oracle()`` / ``gpr()`` build the two sides from them."""

    def __init__(self, d, kid, N, affine=True, normalize_y=True, seed=0, svm=False, s=None, noise_level=1e-2, ymax=None,
                 **kw):
        self.d, self.kid, self.N, self.affine, self.normalize_y, self.svm, self.kw = d, kid, N, affine, normalize_y, svm, kw
        self.noise_level = noise_level
        ll = gauss_ll(d, s=s if s is not None else (0.5 if d <= 5 else 1.5))
        self.bounds, self.X, self.y = training(ll, d, N, seed)
        if ymax is not None:
            # no training point near the mode: the mean rises above the largest training value there
            self.X, self.y = self.X[self.y <= ymax], self.y[self.y <= ymax]
        span = self.bounds[:, 1] - self.bounds[:, 0]
        # length scales of 0.3 in unit-cube coordinates, whichever coordinates the kernel sees
        self.theta = np.log(np.concatenate([[4.0], 0.3 * (np.ones(d) if affine else span)]))
        if svm:
            self.y = self.y.copy()
            self.y[self.X[:, 0] > 1.5] = -np.inf
            self.kw = dict(account_for_inf="SVM", inf_threshold="20s", trust_region_factor=1.5, random_state=1, **kw)

    def gpr(self, device=None):
        g = mirror(self.bounds, self.kid, self.theta, self.affine, self.normalize_y, device=device,
                   noise_level=self.noise_level, **self.kw)
        g.append_to_data(self.X, self.y, fit_gpr=False)
        return g

    def oracle(self, gpr=None):
        """With the SVM the oracle is given the training set the mirror kept (the finite rows)."""
        X, y = (gpr.X_train, gpr.y_train) if self.svm else (self.X, self.y)
        kw = {k: v for k, v in self.kw.items() if k == "clip_factor"}
        return oracle_of(self.bounds, self.kid, self.theta, X, y, self.affine, self.normalize_y,
                         noise_level=self.noise_level, **kw)

    def mean_fn(self, ref, gpr=None):
        """The unclipped oracle mean, -inf where the mirror's host-side masks reject."""
        def mean(X):
            X = np.atleast_2d(X)
            K = orc.kernel_matrix(ref.pre_X.transform(X), ref.theta, ref.kernel_id, Y=ref.X_train_)
            m = ref.pre_y.inverse_transform(K.dot(ref.alpha_))
            if self.svm:
                mask = gpr._masks(X, False, False)
                m = np.where(mask != 0, -np.inf, m)
            return m
        return mean

    def tol(self):
        fin = self.y[np.isfinite(self.y)]
        return MEAN_TOL * max(1.0, float(np.max(np.abs(fin))))


# ---- the table of part A --------------------------------------------------------------------------------------------
RBF, M12, M32, M52 = orc.RBF, orc.MATERN12, orc.MATERN32, orc.MATERN52

# name: (model arguments, variant)
NESTED_CASES = {}
# (d, kernel id, N, affine): every (DP bucket, kernel id) pair once, an odd and an even d in every bucket
PLAIN_ROWS = [(1, RBF, 17, True), (2, M12, 600, False), (3, M52, 600, True), (4, M32, 2048, True),
                           (5, RBF, 600, False), (8, M12, 600, True), (5, M32, 17, True), (8, M52, 4096, False),
                           (9, M52, 600, False), (16, RBF, 2048, True), (16, M12, 17, True), (9, M32, 600, True),
                           (17, M32, 600, True), (32, M52, 600, False), (31, RBF, 600, True), (32, M12, 2048, True)]
for _d, _kid, _N, _aff in PLAIN_ROWS:
    NESTED_CASES[f"d={_d} kid={_kid} N={_N} affine={'on' if _aff else 'off'}"] = (dict(d=_d, kid=_kid, N=_N, affine=_aff), "plain")
_BASE = dict(d=3, kid=M52, N=600)
NESTED_CASES.update({
    "clip active": (dict(d=3, kid=M52, N=400, clip_factor=1.0), "plain"),
    "SVM + trust region": (dict(d=3, kid=M52, N=300, svm=True, seed=9), "plain"),
    "W narrow (1e-3)": (_BASE, "narrow"),
    "W wide (50)": (_BASE, "wide"),
    "plateau": (dict(d=3, kid=M52, N=400, clip_factor=1.0, ymax=-2.0), "plateau"),
    "clustered": (dict(d=5, kid=M52, N=600), "clustered"),
    "volumes": (dict(d=5, kid=M52, N=600), "volumes"),
    "starts on the faces": (_BASE, "faces"),
    "every try gated": (dict(d=3, kid=M52, N=300, svm=True, seed=9), "gated"),
})


class Generation:
    """The inputs of one ``ns_generation`` call of a case, made from the oracle alone (so that the CPU and the GPU file
    run the same walk): 300 prior points of the device's own prior draw, L* at the lowest third's top (the 100th), the rest
    above it the survivors."""

    def __init__(self, name, gpr_device=None):
        from gpry_amd.nested import cholesky_ridged, whitening
        margs, self.variant = NESTED_CASES[name]
        self.name, self.model = name, Model(**margs)
        m, v = self.model, self.variant
        self.gpr = m.gpr(device=gpr_device) if (m.svm or gpr_device is None) else None
        self.ref = m.oracle(self.gpr)
        self.mean = m.mean_fn(self.ref, self.gpr)
        self.clip_hi = float(self.ref.clip_hi())
        d = m.d
        self.seed, self.gen = 1000 + 7 * len(name) + d, 3
        lo, hi = m.bounds[:, 0].copy(), m.bounds[:, 1].copy()
        Xp = prior_points(lo, hi, self.seed, 300)
        yp = np.minimum(self.mean(Xp), self.clip_hi)
        self.labels = self.cum_p = None
        if v == "gated":
            # survivors on rejected ground, with a y the caller vouches for: every try around them meets the gates
            bad = np.flatnonzero(np.isneginf(yp))
            assert len(bad) >= 20, len(bad)
            self.lstar = float(np.sort(yp[np.isfinite(yp)])[100])
            self.Xs, self.ys = Xp[bad], np.full(len(bad), self.lstar + 1.0)
        elif v == "plateau":
            # L* = clip_hi and starts where the unclipped mean lies above it: no try can be accepted, and a box of the
            # plateau's own size, so that tries leave it
            self.lstar = self.clip_hi
            lo, hi = np.full(d, -0.5), np.full(d, 1.1)
            Xq = np.random.default_rng(5).uniform(lo, hi, (2000, d))
            Xq = Xq[self.mean(Xq) > self.clip_hi + 0.1][:40]
            assert len(Xq) == 40
            self.Xs, self.ys = Xq, np.full(40, self.clip_hi)
        else:
            # (prior points the gates reject die first, as in nested.run_nested: L* is taken among the rest)
            order = np.argsort(yp, kind="stable")
            order = order[np.isfinite(yp[order])]
            cut = len(order) // 3
            self.lstar = float(yp[order[cut - 1]])
            self.Xs, self.ys = Xp[order[cut:]], yp[order[cut:]]
        if v == "faces":
            # the box drawn in to the survivors' own extent along the first two coordinates: four of them lie on faces
            lo[:2], hi[:2] = self.Xs[:, :2].min(axis=0), self.Xs[:, :2].max(axis=0)
        self.lo, self.hi = lo, hi
        U = (self.Xs - lo) / (hi - lo)
        W = whitening(U)
        if v in ("narrow", "gated"):
            W = 1e-3 * W
        elif v == "wide":
            W = 50.0 * W
        elif v == "plateau":
            W = 0.5 * np.eye(d)
        elif v in ("clustered", "volumes"):
            rng = np.random.default_rng(2)
            self.labels = rng.integers(0, 3, len(self.Xs)).astype(np.int32)
            Ws = []
            for q in range(3):
                A = rng.normal(size=(d, d))
                Ws.append(cholesky_ridged((0.01 + 0.02 * q) * (A @ A.T / d + 0.1 * np.eye(d))))
            if v == "volumes":
                # cluster 1 has no probability (and no survivor but the relabelled rest), cluster 3 is a single survivor
                self.labels[self.labels == 1] = 0
                self.labels[5] = 3
                self.labels[6] = 1
                Ws.append(cholesky_ridged(0.02 * np.eye(d)))
                self.cum_p = np.array([0.5, 0.5, 0.75, 1.0])
            W = np.stack(Ws)
        self.W = np.ascontiguousarray(W)

    def trace(self, R=R_STEPS, k=N_CHAINS, **kw):
        return traced_generation(self.mean, self.clip_hi, self.lo, self.hi, self.Xs, self.ys, self.lstar, self.W,
                                 self.seed, self.gen, k, R, labels=self.labels, cum_p=self.cum_p, **kw)

    def device_call(self, dev, r, k=N_CHAINS):
        kw = {}
        if self.labels is not None:
            kw["labels"] = self.labels
        if self.cum_p is not None:
            kw["cum_p"] = self.cum_p
        return dev.ns_generation(self.lo, self.hi, self.Xs, self.ys, self.lstar, self.W, self.seed, self.gen, k, r, **kw)

    def min_diag(self):
        W = self.W.reshape(-1, self.model.d, self.model.d)
        return float(np.min(np.abs(np.diagonal(W, axis1=1, axis2=2))))


# ---- the tables of parts B and C ------------------------------------------------------------------------------------
# part B runs the Metropolis rule over PLAIN_ROWS, the instantiations of part A

# part C: every N of the slice layout's edges once, with a d from every DP bucket and every kernel id four times or so
# (a Latin square: row i takes d from _C_D[i % 8], kernel id (i + i // 4) % 4), affine alternating
_C_N = [1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 9217]
_C_D = [1, 8, 16, 32, 4, 5, 9, 17]
EVAL_CASES = [(_C_N[i], _C_D[i % 8], (i + i // 4) % 4, i % 2 == 0) for i in range(len(_C_N))]
# the instantiations the square leaves out, at small N
EVAL_CASES += [(33, d, kid, True) for d in (4, 8, 16, 32) for kid in range(4)
               if (dp_bucket(d), kid) not in {(dp_bucket(c[1]), c[2]) for c in EVAL_CASES}]


def eval_model(N, d, kid, affine):
    """Part C's model: normalize_y off (y_std = 1, y_mean = 0), y of order ten, noise 0.1 (a well-conditioned factor at
    every N, so that the oracle's own rounding stays far below the suite's tolerance)."""
    return Model(d, kid, N, affine=affine, normalize_y=False, seed=N, s=2.0 * np.sqrt(d), noise_level=0.1)


# ---- part B: one Metropolis step restated ---------------------------------------------------------------------------
def check_metropolis_rule(dev, lo, hi, X0, y0, y_start, Lp, T, minus_inf_value, seed, batch, steps, thin, oracle_y=None,
                          oracle_tol=None):
    """Runs ``dev.mcmc_chains(..., proposals=True)`` and checks every step against the rule restated with the numpy
    Philox draws: the proposal is the previous state + (z Lp^T) span to 1e-13 max|bounds|; it is evaluated iff it lies in
    the box; the step is accepted iff y' is finite, above minus_inf_value and log(1 - ua) < (y' - y) / T, exactly, outside
    the borderline steps (|log(1 - ua) - (y' - y) / T| < 1e-12 (1 + |rhs|)); the records, the final state and the counts
    follow.  ``y0``: what the call is given (NaN: the kernel evaluates the start); ``y_start``: the y the rule starts
    from.  ``oracle_y(X)``: a second referee of every evaluated proposal's y.  Returns a dict of counts."""
    import mcmc_numpy
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    span = hi - lo
    n, d = X0.shape
    out = dev.mcmc_chains(lo, hi, X0, y0, Lp, T, minus_inf_value, seed, batch, steps, thin, proposals=True)
    c = np.arange(n)
    X_prev, y_prev = X0, np.asarray(y_start, dtype=float)
    outside = borderline = low = gated = nacc = 0
    tainted = np.zeros(n, bool)              # (thin > 1) chains with a borderline step since the last record
    naccept = np.zeros(n, np.int64)
    atol = 1e-13 * max(np.max(np.abs(lo)), np.max(np.abs(hi)))
    for s in range(steps):
        z = mcmc_numpy.normals(seed, batch, c, s, d)
        Xp, yp = out["X_prop"][:, s], out["y_prop"][:, s]
        if thin == 1 or not tainted.any():
            np.testing.assert_allclose(Xp - X_prev, (z @ np.tril(Lp).T) * span, rtol=0, atol=atol)
        inside = np.all((Xp >= lo) & (Xp <= hi), axis=1)
        np.testing.assert_array_equal(np.isnan(yp), ~inside)
        outside += int(np.sum(~inside))
        if oracle_y is not None and inside.any():
            yo = oracle_y(Xp[inside])
            np.testing.assert_array_equal(np.isneginf(yp[inside]), np.isneginf(yo))
            fin = np.isfinite(yo)
            assert np.max(np.abs(yp[inside][fin] - yo[fin]), initial=0.0) <= oracle_tol
        lu = np.log(1.0 - mcmc_numpy.accept_uniform(seed, batch, c, s))
        with np.errstate(invalid="ignore"):
            rhs = (yp - y_prev) / T
            expect = inside & np.isfinite(yp) & (yp > minus_inf_value) & (lu < rhs)
            close = inside & (np.abs(lu - rhs) < 1e-12 * (1 + np.abs(rhs)))
            low += int(np.sum(inside & np.isfinite(yp) & (yp <= minus_inf_value) & (lu < rhs)))
        gated += int(np.sum(np.isneginf(yp)))
        borderline += int(np.sum(close))
        if thin == 1:
            moved = np.any(out["X"][:, s] != X_prev, axis=1)
            np.testing.assert_array_equal(moved[~close], expect[~close])
            np.testing.assert_array_equal(out["X"][:, s][moved], Xp[moved])
            np.testing.assert_array_equal(out["y"][:, s], np.where(moved, yp, y_prev))
            X_prev, y_prev = out["X"][:, s], out["y"][:, s]
            naccept += moved
        else:
            tainted |= close
            X_prev = np.where(expect[:, None], Xp, X_prev)
            y_prev = np.where(expect, yp, y_prev)
            naccept += expect
            if (s + 1) % thin == 0:
                r = (s + 1) // thin - 1
                ok = ~tainted
                np.testing.assert_array_equal(out["X"][:, r][ok], X_prev[ok])
                np.testing.assert_array_equal(out["y"][:, r][ok], y_prev[ok])
    assert borderline < 3
    assert out["X"].shape == (n, steps // thin, d)
    if thin == 1:
        moves = np.any(np.diff(np.concatenate([X0[:, None], out["X"]], axis=1), axis=1) != 0, axis=2)
        np.testing.assert_array_equal(out["naccept"], moves.sum(axis=1))
        if steps:
            np.testing.assert_array_equal(out["X_last"], out["X"][:, -1])
    ok = ~tainted
    np.testing.assert_array_equal(out["naccept"][ok], naccept[ok])
    np.testing.assert_array_equal(out["X_last"][ok], X_prev[ok])
    np.testing.assert_array_equal(out["y_last"][ok], y_prev[ok])
    np.testing.assert_array_equal(out["ncalls"], np.isnan(y0).astype(np.int64) + np.sum(~np.isnan(out["y_prop"]), axis=1))
    return dict(outside=outside, borderline=borderline, below_minus_inf_value=low, gated=gated,
                accepted=int(out["naccept"].sum()))
