"""numpy stand-in for the device call of gpry_amd/hmc.py (``dev.hmc_chains``, kernel in gpry_amd/csrc/hmc.hip), the
trajectory-by-trajectory host reference the GPU walk test checks the kernel against, and that test's table of cases.

``HmcNumpyDevice(loglike, grad_x)``: the device's algorithm on a numpy log-density ``loglike(X (m, d)) -> (m,)`` (what
the acceptance sees: for a surrogate, clip and gates included) and its raw-coordinate gradient ``grad_x(X) -> (m, d)``
(for a surrogate: of the unclipped, ungated mean) -- the same Philox counters (phase 4, draw j, batch, chain,
trajectory; j < 16: z, 16: acceptance, 17: step-size jitter), the same leapfrog, box test and acceptance rule, chains
vectorised: the same distribution as the device, not the same bits.  ``oracle_grad_x(ref)`` is the gradient of the
float64 numpy oracle's mean, for a stand-in or a trace on the oracle.

``traced_trajectories``: the same algorithm, keeping per chain c and trajectory s the last point reached (``U``, ``X``:
the end point, or where the trajectory was cut short), ``y`` and ``dH`` (NaN where nothing was evaluated), the decision
``accepted``, ``margin_face`` (the smallest distance of any drift of the trajectory from the faces 0 and 1 of the cube)
and ``margin_acc`` (|log(1 - ua) - dH|; inf where nothing was evaluated), and the running counts.

Arithmetic.  ``dtype=np.longdouble`` runs the same trajectories (same draws; log-density and gradient still float64
functions of the float64-rounded point) in extended precision.  The largest |U_float64 - U_longdouble| of the end points
over the chains x trajectories the margins keep, over the whole table HMC_CASES, is the arithmetic noise floor of the
restatement: eps_h = 2.78e-15 measured (x86 80-bit long double), rounded up to EPS_H = 3e-15 below;
tests/test_hmc_cpu.py measures it again on every run and asserts it stays below EPS_H.  The GPU test allows
POS_TOL = 100 x EPS_H = 3e-13: two orders for what the kernel does differently (the order of its sums, the device's
log / cos / sin, and its gradient, which agrees with the oracle's to rounding and not to the bit).

Which chains are compared: those whose every decision so far has margin_acc > ACC_MARGIN = 1e-9 and margin_face >
FACE_MARGIN = 1e-9; the others are left out from that trajectory on and counted.  At most 25 % of a case's chains and 5 %
of the table's may be left out (LEFT_OUT_CASE, LEFT_OUT_TABLE)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ns_philox import philox  # noqa: E402

PHASE_HMC, DRAW_ACCEPT, DRAW_JITTER = 4, 16, 17
EPS_H = 3e-15
POS_TOL = 100 * EPS_H
ACC_MARGIN = FACE_MARGIN = 1e-9
LEFT_OUT_CASE, LEFT_OUT_TABLE = 0.25, 0.05
N_TRAJ, N_CHAINS, N_LEAP = 8, 64, 5


def normals(seed, batch, chains, step, d, dtype=np.float64):
    """z (len(chains), d) of trajectory ``step``: Box-Muller of draws 0..(d-1)/2, as the kernel does."""
    h = (d + 1) // 2
    chains = np.asarray(chains)
    ua, ub = philox(seed, PHASE_HMC, np.arange(h)[None, :], batch, chains[:, None], step)
    ua, ub = ua.astype(dtype), ub.astype(dtype)
    two_pi = 2 * np.pi if dtype is np.float64 else 8 * np.arctan(dtype(1))
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - ua)), two_pi * ub
    z = np.empty((len(chains), 2 * h), dtype=dtype)
    z[:, 0::2], z[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
    return z[:, :d]


def accept_uniform(seed, batch, chains, step):
    return philox(seed, PHASE_HMC, DRAW_ACCEPT, batch, np.asarray(chains), step)[0]


def jitter_uniform(seed, batch, chains, step):
    return philox(seed, PHASE_HMC, DRAW_JITTER, batch, np.asarray(chains), step)[0]


def leapfrog(grad_u, lo, span, u, g, p, Lp, eps_s, nleap, T, dtype=np.float64):
    """``nleap`` leapfrog steps of the chains (u, p) (n, d) with step sizes eps_s (n,), g = grad_u at u:
    ``(u', x', g', p', alive, face, ngrad)``.  A chain whose drift leaves the box or whose gradient is not finite stops
    there (alive False; u', x' are where it stopped); face: the smallest distance of its drifts from the faces."""
    n, d = u.shape
    L = np.tril(np.asarray(Lp, dtype=float)).astype(dtype)
    lo_, hi_ = lo, lo + span
    u, p, g = u.copy(), p.copy(), np.asarray(g, dtype=float).copy()
    x = lo + u * span
    face = np.full(n, np.inf)
    ngrad = np.zeros(n, np.int64)
    alive = np.all(np.isfinite(g), axis=1)
    e = eps_s[:, None]
    p[alive] = (p + (0.5 * e / T) * (g.astype(dtype) @ L))[alive]
    for l in range(nleap):
        if not alive.any():
            break
        un = u + e * (p @ L.T)
        xn = lo + un * span
        u[alive], x[alive] = un[alive], xn[alive]
        f = np.min(np.minimum(np.abs(un), np.abs(un - 1)), axis=1).astype(float)
        face[alive] = np.minimum(face[alive], f[alive])
        alive = alive & np.all((un >= 0) & (un <= 1) & (xn >= lo_) & (xn <= hi_), axis=1)
        if not alive.any():
            break
        gn = np.asarray(grad_u(np.ascontiguousarray(x[alive].astype(float))), dtype=float)
        g[alive] = gn
        ngrad[alive] += 1
        alive[alive] = np.all(np.isfinite(gn), axis=1)
        kick = (0.5 if l == nleap - 1 else 1.0) * e / T
        p[alive] = (p + kick * (g.astype(dtype) @ L))[alive]
    return u, x, g, p, alive, face, ngrad


class Trace:
    def __init__(self, n, nsteps, d):
        self.U, self.X = np.empty((nsteps, n, d)), np.empty((nsteps, n, d))
        self.y, self.dH = np.full((nsteps, n), np.nan), np.full((nsteps, n), np.nan)
        self.accepted = np.zeros((nsteps, n), bool)
        self.margin_face, self.margin_acc = np.full((nsteps, n), np.inf), np.full((nsteps, n), np.inf)
        self.ncalls, self.ngrad = np.zeros((nsteps, n), np.int64), np.zeros((nsteps, n), np.int64)

    def keep(self, s):
        """The chains whose decisions up to and including trajectory s all lie outside the margins."""
        return (np.min(self.margin_acc[:s + 1], axis=0) > ACC_MARGIN) & (np.min(self.margin_face[:s + 1], axis=0) > FACE_MARGIN)


def _run(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, dtype=np.float64,
         chains=None):
    """The algorithm of hmc_chain_kernel; returns (out dict of ``hmc_chains`` with the hooks, Trace)."""
    ft = dtype
    lo64, hi64 = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    lo_, span = lo64.astype(ft), (hi64 - lo64).astype(ft)
    X0 = np.asarray(X0, dtype=float)
    n, d = X0.shape
    if not (T > 0 and np.isfinite(T)):
        raise ValueError(f"temperature T = {T}")
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"step size eps = {eps}")
    if not 1 <= nleap <= 1024:
        raise ValueError(f"nleap = {nleap}")
    c = np.arange(n) if chains is None else np.asarray(chains)
    span64 = hi64 - lo64

    def grad_u(X):
        return np.asarray(grad_x(X), dtype=float) * span64

    x = X0.astype(ft)
    u = (x - lo_) / span
    y = np.asarray(y0, dtype=float).copy()
    cnt, nacc = np.zeros(n, np.int64), np.zeros(n, np.int64)
    todo = np.isnan(y)
    if todo.any():
        y[todo] = loglike(X0[todo])
        cnt[todo] += 1
    g = grad_u(X0)
    ng = np.ones(n, np.int64)
    G0 = g.copy()
    nrec = nsteps // thin
    Xr, yr = np.empty((n, nrec, d)), np.empty((n, nrec))
    tr = Trace(n, nsteps, d)
    for s in range(nsteps):
        p0 = normals(seed, batch, c, s, d, ft)
        eps_s = (eps * (0.8 + 0.4 * jitter_uniform(seed, batch, c, s))).astype(ft)
        ut, xt, gt, p1, alive, face, ngs = leapfrog(grad_u, lo_, span, u, g, p0, Lp, eps_s, nleap, T, ft)
        ng += ngs
        yt, dH = np.full(n, np.nan), np.full(n, np.nan)
        if alive.any():
            yt[alive] = loglike(np.ascontiguousarray(xt[alive].astype(float)))
            cnt[alive] += 1
            with np.errstate(invalid="ignore"):
                dH[alive] = ((yt - y) / T - 0.5 * (np.sum(p1 * p1, axis=1) - np.sum(p0 * p0, axis=1)).astype(float))[alive]
        lu = np.log(1.0 - accept_uniform(seed, batch, c, s))
        with np.errstate(invalid="ignore"):
            acc = alive & np.isfinite(yt) & (yt > minus_inf_value) & (lu < dH)
            tr.margin_acc[s] = np.where(alive & np.isfinite(dH), np.abs(lu - dH), np.inf)
        tr.U[s], tr.X[s], tr.y[s], tr.dH[s], tr.accepted[s], tr.margin_face[s] = ut.astype(float), xt.astype(float), yt, dH, acc, face
        x[acc], u[acc], y[acc], g[acc] = xt[acc], ut[acc], yt[acc], gt[acc]
        nacc += acc
        tr.ncalls[s], tr.ngrad[s] = cnt, ng
        if (s + 1) % thin == 0:
            Xr[:, (s + 1) // thin - 1], yr[:, (s + 1) // thin - 1] = x.astype(float), y
    out = dict(X=Xr, y=yr, X_last=x.astype(float), y_last=y, naccept=nacc, ncalls=cnt, ngrad=ng, device_ms=0.0,
               X_prop=np.ascontiguousarray(tr.X.transpose(1, 0, 2)), y_prop=tr.y.T.copy(), dH_prop=tr.dH.T.copy(), G0=G0)
    return out, tr


def traced_trajectories(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps,
                        dtype=np.float64):
    """The trace (see the module's docstring) of ``hmc_chains(lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed,
    batch, nsteps, 1)``."""
    return _run(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, 1, dtype)[1]


class HmcNumpyDevice:
    """``hmc_chains`` of gpry_amd/_lib.py on a numpy log-density and its gradient; keeps the arguments of every call in
    ``calls``."""

    def __init__(self, loglike, grad_x):
        self.loglike, self.grad_x = loglike, grad_x
        self.calls = []

    def hmc_chains(self, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, hooks=False,
                   chains=None):
        """``chains``: the chain numbers the rows of X0 stand for (default 0 .. n - 1): what chain c of a wider call
        draws."""
        self.calls.append(dict(batch=batch, nsteps=nsteps, thin=thin, Lp=np.array(Lp), eps=eps, nleap=nleap, T=T,
                               nchains=len(X0)))
        out, _ = _run(self.loglike, self.grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps,
                      thin, chains=chains)
        if not hooks:
            for k in ("X_prop", "y_prop", "dH_prop", "G0"):
                del out[k]
        return out


# ---- the oracle's mean gradient -------------------------------------------------------------------------------------
def oracle_grad_x(ref):
    """Raw-coordinate gradient of the oracle's unclipped mean: the gradient in the kernel's coordinates
    (``kernel_gradient_x``, y_std included), divided by the span of the x-affine map where there is one."""
    from oracle import gpry_oracle as orc
    xspan = (ref.pre_X.hi - ref.pre_X.lo) if hasattr(ref.pre_X, "hi") else 1.0

    def grad_x(X):
        X_ = ref.pre_X.transform(np.atleast_2d(X))
        G = np.array([orc.kernel_gradient_x(x_, ref.X_train_, ref.theta, ref.kernel_id).T.dot(ref.alpha_) for x_ in X_])
        return ref.pre_y.inverse_transform_scale(G.reshape(len(X_), -1)) / xspan
    return grad_x


# ---- the walk table -------------------------------------------------------------------------------------------------
# kernels x d in {3, 16} x N in {100, 1100} (one ragged slice, one slice of 1100 rows), a gated and a tempered case
def _cases():
    import sampler_walk as sw
    cases = {}
    for kid in (sw.RBF, sw.M12, sw.M32, sw.M52):
        for d in (3, 16):
            for N in (100, 1100):
                cases[f"kid={kid} d={d} N={N}"] = (dict(d=d, kid=kid, N=N, affine=(kid + d + N // 1000) % 2 == 0), 1.0)
    cases["gated"] = (dict(d=3, kid=sw.M52, N=300, svm=True, seed=9), 1.0)
    cases["tempered"] = (dict(d=3, kid=sw.M52, N=600), 2.0)
    return cases


class Walk:
    """The inputs of one ``hmc_chains`` call of a case, made from the oracle alone, so that the CPU and the GPU file run
    the same trajectories.  Model: ``sampler_walk.Model`` with normalize_y off and noise 0.1 (``eval_model``'s reasons: a
    well-conditioned factor, so that the oracle's and the device's alpha agree far below the position tolerance: a
    difference dg of the two gradients moves an end point by about eps^2 Lp Lp^T dg per step).  Starts: training rows near
    the mode.  Lp: the Cholesky factor of the starts' covariance in the unit cube; eps = 0.25."""

    def __init__(self, name, gpr_device=None):
        import sampler_walk as sw
        from gpry_amd.nested import cholesky_ridged
        margs, self.T = _cases()[name]
        margs = dict(margs)
        d = margs["d"]
        self.name = name
        self.model = m = sw.Model(normalize_y=False, noise_level=0.1, s=0.5 * np.sqrt(d), **margs)
        self.gpr = m.gpr(device=gpr_device) if (m.svm or gpr_device is None) else None
        self.ref = m.oracle(self.gpr)
        mean = m.mean_fn(self.ref, self.gpr)
        clip = float(self.ref.clip_hi())
        self.loglike = lambda X: np.minimum(mean(X), clip)
        self.grad_x = oracle_grad_x(self.ref)
        self.lo, self.hi = m.bounds[:, 0].copy(), m.bounds[:, 1].copy()
        X, y = (self.gpr.X_train, self.gpr.y_train) if m.svm else (m.X, m.y)
        order = np.argsort(-y, kind="stable")[:N_CHAINS]
        self.X0 = np.ascontiguousarray(X[order])
        U = (self.X0 - self.lo) / (self.hi - self.lo)
        self.Lp = cholesky_ridged(np.atleast_2d(np.cov(U, rowvar=False, ddof=0)))
        self.eps, self.seed, self.batch = 0.25, 2000 + 7 * len(name) + d, 3
        self.minus_inf_value = -np.inf

    def args(self):
        return (self.lo, self.hi, self.X0, np.full(len(self.X0), np.nan), self.Lp, self.eps, N_LEAP, self.T,
                self.minus_inf_value, self.seed, self.batch, N_TRAJ)

    def trace(self, **kw):
        return traced_trajectories(self.loglike, self.grad_x, *self.args(), **kw)


HMC_CASES = list(_cases())
