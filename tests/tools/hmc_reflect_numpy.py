"""numpy restatement of the reflective drift of the device's HMC (``hmc_chains(..., reflect=True)``, kernel
``hmc_chain_kernel<DP, KID, true>`` in gpry_amd/csrc/hmc.hip), a stand-in for that device call, the traced reference the
GPU walk test checks the kernel against, and that test's table of cases.  Built on tests/tools/hmc_numpy.py: the draws,
the kicks, the acceptance rule and the records are its own.

The drift (include/gpry_hip.h, gpry_hmc_chains_reflect): a billiard flow of duration tau = eps_s inside [0, 1]^d.  With
v = Lp p: the hit times t_k = ((v_k > 0) - u_k) / v_k (inf for v_k = 0) and j, the lowest index with the smallest; without
a hit before tau, u += tau v ends the drift; otherwise u += t_j v with u_j set on its wall, p -= (2 a / b) r with r = row j
of Lp, a = r . p = v_j, b = r . r, tau -= t_j; u is clamped to [0, 1] after every move and x to [lo, hi] after the drift.  A
drift that has made ``max_reflect`` reflections and meets another wall rejects the trajectory where it stands.

``HmcReflectNumpyDevice``: ``hmc_numpy.HmcNumpyDevice`` with ``reflect=False, max_reflect=64``; with ``reflect`` the dict
gains ``nreflect``.  With ``reflect`` off it runs ``hmc_numpy.leapfrog`` and returns that stand-in's bits.

``traced_trajectories``: as ``hmc_numpy.traced_trajectories``; beside ``margin_acc`` the trace keeps, per chain and
trajectory, the smallest over the trajectory's drifts of
- ``margin_hit``: |tau - t_j| |v_j| at every reflect-or-not decision (inf where no coordinate moves);
- ``margin_wall``: (t_j' - t_j) max(|v_j|, |v_j'|), j' the runner-up, at every reflection (which wall: small near a
  corner);
- ``margin_cap``: max_reflect minus the reflections of the drift (0: the cap was reached);
and ``nrefl`` (the reflections of the trajectory), ``maxdrift`` (the most of a single drift of it) and ``nreflect`` (the
running count).  ``margin_face`` is inf: with reflection no decision hangs on the distance from a face.

Which chains are compared: those whose every decision so far has margin_acc > 1e-9 (``hmc_numpy.ACC_MARGIN``) and all
three margins above > MARGIN = 1e-9; the others are left out from that trajectory on and counted, under ``hmc_numpy``'s
caps (25 % of a case's chains, 5 % of the table's).

Arithmetic.  As in ``hmc_numpy``: the largest |U_float64 - U_longdouble| of the end points over the kept chains x
trajectories of the whole table REFLECT_CASES is the noise floor of the restatement: eps_h = 4.72e-14 measured (x86 80-bit
long double; a reflection turns a rounding of the hit time into one of the momentum), rounded up to EPS_H = 5e-14; tests/test_hmc_reflect_cpu.py measures it again on every run.  The GPU test
allows POS_TOL = 100 x EPS_H.

The table (64 chains, 8 trajectories, 5 leapfrog steps): d in {2, 5, 16, 32} x {RBF, Matern-5/2}, N alternating between 100
and 1100, a gated, a tempered and a corner case.  Every call's box is [-0.9, 1.9]^d inside the models' [-4, 4]^d, off the
mode at 0.3; the starts are uniform draws in it (for the gated case: those on accepted ground), so every wall lies within
1.7 standard deviations of the starts' centre; Lp is the Cholesky factor of the starts' covariance in the unit cube, eps =
EPS_TABLE = 0.7 (a drift of 0.2 box widths per unit of momentum: at d = 2 a third of the trajectories meet a wall, from
d = 16 on all do).  The corner case starts within 5 % of the box from the corner at lo, with the Lp scale of starts that
fill the box and eps = EPS_CORNER = 0.75: a drift towards the corner meets two or three walls."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmc_numpy as hn  # noqa: E402
from hmc_numpy import LEFT_OUT_CASE, LEFT_OUT_TABLE, N_CHAINS, N_LEAP, N_TRAJ  # noqa: E402,F401

EPS_H = 5e-14
POS_TOL = 100 * EPS_H
MARGIN = 1e-9
MAX_REFLECT = 64


def billiard(u, p, L, tau, active, max_reflect, dtype=np.float64):
    """The reflective drift of the rows ``active`` of (u, p) (n, d), in place, for the times tau (n,):
    ``(capped, nrefl, margin_hit, margin_wall)``, per chain: whether the cap cut the drift short, its reflections and the
    smallest margins of its decisions."""
    n, d = u.shape
    rows = np.arange(n)
    tau = tau.astype(dtype).copy()
    todo = active.copy()
    capped, nrefl = np.zeros(n, bool), np.zeros(n, np.int64)
    m_hit, m_wall = np.full(n, np.inf), np.full(n, np.inf)
    zero, one = dtype(0), dtype(1)
    while todo.any():
        v = p @ L.T
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            th = np.where(v != 0, (np.where(v > 0, one, zero) - u) / v, np.inf)
        th = np.where(np.isnan(th), np.inf, th)
        j = np.argmin(th, axis=1)                     # (the first of equal ones: the lowest index)
        tj, vj = th[rows, j], v[rows, j]
        hit = todo & (tj < tau)
        with np.errstate(invalid="ignore"):
            mh = np.where(np.isfinite(tj), np.abs(tau - tj) * np.abs(vj), np.inf).astype(float)
        m_hit[todo] = np.minimum(m_hit[todo], mh[todo])
        if d > 1:
            th2 = th.copy()
            th2[rows, j] = np.inf
            j2 = np.argmin(th2, axis=1)
            with np.errstate(invalid="ignore"):
                mw = np.where(np.isfinite(th2[rows, j2]),
                              (th2[rows, j2] - tj) * np.maximum(np.abs(vj), np.abs(v[rows, j2])), np.inf).astype(float)
            m_wall[hit] = np.minimum(m_wall[hit], mw[hit])
        done = todo & ~hit
        un = u + tau[:, None] * v
        u[done] = np.where(un < 0, zero, np.where(un > 1, one, un))[done]
        cap = hit & (nrefl == max_reflect)
        capped |= cap
        do = hit & ~cap
        if do.any():
            um = u + tj[:, None] * v
            um[rows, j] = np.where(vj > 0, one, zero)
            u[do] = np.where(um < 0, zero, np.where(um > 1, one, um))[do]
            r = L[j]                                  # (lower triangular: the entries beyond j are zero)
            b = np.sum(r * r, axis=1)
            p[do] = (p - ((2.0 * vj) / b)[:, None] * r)[do]
            tau = np.where(do, tau - tj, tau)
            nrefl += do
        todo = do
    return capped, nrefl, m_hit, m_wall


def leapfrog(grad_u, lo, span, u, g, p, Lp, eps_s, nleap, T, max_reflect=MAX_REFLECT, dtype=np.float64):
    """``hmc_numpy.leapfrog`` with the reflective drift: ``(u', x', g', p', alive, stats, ngrad)``; a chain whose drift
    runs into the cap or whose gradient is not finite stops there.  stats: dict of per-chain ``nrefl`` (reflections),
    ``maxdrift`` (the most in one drift), ``margin_hit``, ``margin_wall``, ``margin_cap`` and ``dp2`` (the largest change
    of |p|^2 across a drift)."""
    n, d = u.shape
    L = np.tril(np.asarray(Lp, dtype=float)).astype(dtype)
    lo_, hi_ = lo, lo + span
    u, p, g = u.copy(), p.copy(), np.asarray(g, dtype=float).copy()
    x = lo + u * span
    st = dict(nrefl=np.zeros(n, np.int64), maxdrift=np.zeros(n, np.int64), margin_hit=np.full(n, np.inf),
              margin_wall=np.full(n, np.inf), margin_cap=np.full(n, np.inf), dp2=np.zeros(n))
    ngrad = np.zeros(n, np.int64)
    alive = np.all(np.isfinite(g), axis=1)
    e = eps_s[:, None]
    p[alive] = (p + (0.5 * e / T) * (g.astype(dtype) @ L))[alive]
    for l in range(nleap):
        if not alive.any():
            break
        p2 = np.sum(p * p, axis=1)
        capped, nr, mh, mw = billiard(u, p, L, eps_s, alive, max_reflect, dtype)
        st["dp2"][alive] = np.maximum(st["dp2"], np.abs(np.sum(p * p, axis=1) - p2).astype(float))[alive]
        st["nrefl"] += nr
        st["maxdrift"] = np.maximum(st["maxdrift"], nr)
        st["margin_hit"] = np.minimum(st["margin_hit"], mh)
        st["margin_wall"] = np.minimum(st["margin_wall"], mw)
        st["margin_cap"][alive] = np.minimum(st["margin_cap"], (max_reflect - nr).astype(float))[alive]
        xn = lo + u * span
        xn = np.where(xn < lo_, lo_, np.where(xn > hi_, hi_, xn))
        x[alive] = xn[alive]
        alive = alive & ~capped & np.all((u >= 0) & (u <= 1) & (xn >= lo_) & (xn <= hi_), axis=1)
        if not alive.any():
            break
        gn = np.asarray(grad_u(np.ascontiguousarray(x[alive].astype(float))), dtype=float)
        g[alive] = gn
        ngrad[alive] += 1
        alive[alive] = np.all(np.isfinite(gn), axis=1)
        kick = (0.5 if l == nleap - 1 else 1.0) * e / T
        p[alive] = (p + kick * (g.astype(dtype) @ L))[alive]
    return u, x, g, p, alive, st, ngrad


class Trace(hn.Trace):
    def __init__(self, n, nsteps, d):
        super().__init__(n, nsteps, d)
        self.margin_hit, self.margin_wall = np.full((nsteps, n), np.inf), np.full((nsteps, n), np.inf)
        self.margin_cap = np.full((nsteps, n), np.inf)
        self.nrefl, self.maxdrift = np.zeros((nsteps, n), np.int64), np.zeros((nsteps, n), np.int64)
        self.nreflect = np.zeros((nsteps, n), np.int64)

    def keep(self, s):
        ok = super().keep(s)
        for m in (self.margin_hit, self.margin_wall, self.margin_cap):
            ok = ok & (np.min(m[:s + 1], axis=0) > MARGIN)
        return ok


def _run(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, dtype=np.float64,
         chains=None, reflect=False, max_reflect=MAX_REFLECT):
    """``hmc_numpy._run`` with the drift of choice; returns (out dict of ``hmc_chains`` with the hooks, Trace)."""
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
    if reflect and not 1 <= max_reflect <= 1024:
        raise ValueError(f"max_reflect = {max_reflect}")
    c = np.arange(n) if chains is None else np.asarray(chains)
    span64 = hi64 - lo64

    def grad_u(X):
        return np.asarray(grad_x(X), dtype=float) * span64

    x = X0.astype(ft)
    u = (x - lo_) / span
    y = np.asarray(y0, dtype=float).copy()
    cnt, nacc, nrf = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
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
        p0 = hn.normals(seed, batch, c, s, d, ft)
        eps_s = (eps * (0.8 + 0.4 * hn.jitter_uniform(seed, batch, c, s))).astype(ft)
        if reflect:
            ut, xt, gt, p1, alive, st, ngs = leapfrog(grad_u, lo_, span, u, g, p0, Lp, eps_s, nleap, T, max_reflect, ft)
            nrf += st["nrefl"]
            tr.margin_hit[s], tr.margin_wall[s], tr.margin_cap[s] = st["margin_hit"], st["margin_wall"], st["margin_cap"]
            tr.nrefl[s], tr.maxdrift[s] = st["nrefl"], st["maxdrift"]
        else:
            ut, xt, gt, p1, alive, face, ngs = hn.leapfrog(grad_u, lo_, span, u, g, p0, Lp, eps_s, nleap, T, ft)
            tr.margin_face[s] = face
        ng += ngs
        yt, dH = np.full(n, np.nan), np.full(n, np.nan)
        if alive.any():
            yt[alive] = loglike(np.ascontiguousarray(xt[alive].astype(float)))
            cnt[alive] += 1
            with np.errstate(invalid="ignore"):
                dH[alive] = ((yt - y) / T - 0.5 * (np.sum(p1 * p1, axis=1) - np.sum(p0 * p0, axis=1)).astype(float))[alive]
        lu = np.log(1.0 - hn.accept_uniform(seed, batch, c, s))
        with np.errstate(invalid="ignore"):
            acc = alive & np.isfinite(yt) & (yt > minus_inf_value) & (lu < dH)
            tr.margin_acc[s] = np.where(alive & np.isfinite(dH), np.abs(lu - dH), np.inf)
        tr.U[s], tr.X[s], tr.y[s], tr.dH[s], tr.accepted[s] = ut.astype(float), xt.astype(float), yt, dH, acc
        x[acc], u[acc], y[acc], g[acc] = xt[acc], ut[acc], yt[acc], gt[acc]
        nacc += acc
        tr.ncalls[s], tr.ngrad[s], tr.nreflect[s] = cnt, ng, nrf
        if (s + 1) % thin == 0:
            Xr[:, (s + 1) // thin - 1], yr[:, (s + 1) // thin - 1] = x.astype(float), y
    out = dict(X=Xr, y=yr, X_last=x.astype(float), y_last=y, naccept=nacc, ncalls=cnt, ngrad=ng, device_ms=0.0,
               X_prop=np.ascontiguousarray(tr.X.transpose(1, 0, 2)), y_prop=tr.y.T.copy(), dH_prop=tr.dH.T.copy(), G0=G0)
    if reflect:
        out["nreflect"] = nrf
    return out, tr


def traced_trajectories(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps,
                        dtype=np.float64, max_reflect=MAX_REFLECT):
    """The trace of ``hmc_chains(lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, 1,
    reflect=True, max_reflect=max_reflect)``."""
    return _run(loglike, grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, 1, dtype,
                reflect=True, max_reflect=max_reflect)[1]


class HmcReflectNumpyDevice:
    """``hmc_chains`` of gpry_amd/_lib.py, ``reflect`` and ``max_reflect`` included, on a numpy log-density and its
    gradient; keeps the arguments of every call in ``calls``."""

    def __init__(self, loglike, grad_x):
        self.loglike, self.grad_x = loglike, grad_x
        self.calls = []

    def hmc_chains(self, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, hooks=False,
                   chains=None, reflect=False, max_reflect=MAX_REFLECT):
        self.calls.append(dict(batch=batch, nsteps=nsteps, thin=thin, Lp=np.array(Lp), eps=eps, nleap=nleap, T=T,
                               nchains=len(X0), reflect=reflect, max_reflect=max_reflect))
        out, _ = _run(self.loglike, self.grad_x, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps,
                      thin, chains=chains, reflect=reflect, max_reflect=max_reflect)
        if not hooks:
            for k in ("X_prop", "y_prop", "dH_prop", "G0"):
                del out[k]
        return out


# ---- the walk table -------------------------------------------------------------------------------------------------
BOX = (-0.9, 1.9)
EPS_TABLE, EPS_CORNER = 0.7, 0.75


def _cases():
    import sampler_walk as sw
    cases = {}
    i = 0
    for d in (2, 5, 16, 32):
        for kid in (sw.RBF, sw.M52):
            N = (100, 1100)[i % 2]
            cases[f"kid={kid} d={d} N={N}"] = (dict(d=d, kid=kid, N=N, affine=(i // 2) % 2 == 0), 1.0, "plain")
            i += 1
        i += 1                                          # (so that each kernel meets both N)
    cases["gated"] = (dict(d=3, kid=sw.M52, N=300, svm=True, seed=9), 1.0, "gated")
    cases["tempered"] = (dict(d=3, kid=sw.M52, N=600), 2.0, "plain")
    cases["corner"] = (dict(d=3, kid=sw.M52, N=600), 1.0, "corner")
    return cases


class Walk:
    """The inputs of one ``hmc_chains(..., reflect=True)`` call of a case, made from the oracle alone (``hmc_numpy.Walk``'s
    models); see the module's docstring for the box, the starts, Lp and eps."""

    def __init__(self, name, gpr_device=None):
        import sampler_walk as sw
        from gpry_amd.nested import cholesky_ridged
        margs, self.T, variant = _cases()[name]
        margs = dict(margs)
        d = margs["d"]
        self.name = name
        self.model = m = sw.Model(normalize_y=False, noise_level=0.1, s=0.5 * np.sqrt(d), **margs)
        self.gpr = m.gpr(device=gpr_device) if (m.svm or gpr_device is None) else None
        self.ref = m.oracle(self.gpr)
        mean = m.mean_fn(self.ref, self.gpr)
        clip = float(self.ref.clip_hi())
        self.loglike = lambda X: np.minimum(mean(X), clip)
        self.grad_x = hn.oracle_grad_x(self.ref)
        self.lo, self.hi = np.full(d, BOX[0]), np.full(d, BOX[1])
        rng = np.random.default_rng(100 + 7 * len(name) + d)
        U = rng.uniform(0.0, 0.05 if variant == "corner" else 1.0, (4 * N_CHAINS, d))
        X = self.lo + U * (self.hi - self.lo)
        if variant == "gated":
            X = X[np.isfinite(self.loglike(X))]
        self.X0 = np.ascontiguousarray(X[:N_CHAINS])
        assert len(self.X0) == N_CHAINS
        U = (self.X0 - self.lo) / (self.hi - self.lo)
        C = np.atleast_2d(np.cov(U, rowvar=False, ddof=0))
        if variant == "corner":
            C = C * (1.0 / 12.0) / np.mean(np.diag(C))          # (the scale of starts that fill the box)
        self.Lp = cholesky_ridged(C)
        self.eps = EPS_CORNER if variant == "corner" else EPS_TABLE
        self.seed, self.batch = 3000 + 7 * len(name) + d, 3
        self.minus_inf_value = -np.inf
        self.max_reflect = MAX_REFLECT

    def args(self):
        return (self.lo, self.hi, self.X0, np.full(len(self.X0), np.nan), self.Lp, self.eps, N_LEAP, self.T,
                self.minus_inf_value, self.seed, self.batch, N_TRAJ)

    def trace(self, **kw):
        return traced_trajectories(self.loglike, self.grad_x, *self.args(), max_reflect=self.max_reflect, **kw)


REFLECT_CASES = list(_cases())
