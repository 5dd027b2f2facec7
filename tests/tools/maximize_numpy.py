"""numpy stand-in for the device call of gpry_amd/maximize.py (``dev.maximize_mean``, kernel in
gpry_amd/csrc/maximize.hip), the iteration-by-iteration replay the GPU walk test checks the kernel against, and that
test's table of cases.

``MaxNumpyDevice(loglike, grad_x)``: the device's algorithm (include/gpry_hip.h: gpry_maximize_mean) on a numpy
log-density ``loglike(X (m, d)) -> (m,)`` (for a surrogate: clip and gates included) and its raw-coordinate gradient
``grad_x(X) -> (m, d)`` (of the unclipped, ungated mean), starts vectorised: the same free sets, directions, searches,
updates and stops in the same order of operations -- the same decisions as the device, not the same bits (the values
and gradients differ at rounding level).

``replay(trace, lo, hi, X0, fixed, H0, max_iter, max_halvings, gtol, ftol, minus_inf_value, value_of, dtype)``: for every
start and every iteration i of a trace (the dict of ``maximize_mean(..., hooks=True)``) the iterate i + 1 recomputed from
the trace's own ``U_tr[<= i]``, ``G_tr[<= i]`` and ``y_tr[i]``: H is rebuilt from the traced history with the device's
formulas in the device's order (its resets are the trace's ``reset_tr``), and the y of every trial point is taken from
``value_of(X (m, d)) -> (m,)``.  On the GPU ``value_of`` is the one-point ``gpr.predict``, which ns_eval equals bit for
bit: the replay then sees the kernel's exact y and gradients, and the comparison isolates the kernel's own algebra (free
set, direction, clamp, search, update, stops).  Returned, per start and iteration: ``U_next``, ``nhalv``, ``reset``
(what the device's ``U_tr[i + 1]``, ``nhalv_tr[i]``, ``reset_tr[i]`` should be), ``ran`` (the iteration reached its
search), ``end_iters`` / ``end_status`` (-1 where the replay does not see the trace end where it ended), and the margin of
every decision taken:

- Armijo: |y' - y - c1 sum g du| / max(1, |y|) of every evaluated trial with a finite y' (a superset of "the accepted
  trial and the last rejected one"; a gated trial, -inf, has none);
- free set: min |g_k| over the coordinates on a wall that are not fixed;
- direction: p.g / (|p| |g|) (its sign decides a reset);
- curvature: |sq - 1e-10 |s||q|| / (|s||q|); it decides the H of the iterations after, so a start is left out from the
  iteration after a small one on, until H is reset;
- the two stop tests: |max|g| - gtol| and |y' - y - ftol max(1, |y'|)| (where ftol > 0; with ftol = 0 an accepted step
  has y' > y by the Armijo margin).

``margin[c, i]`` is the smallest of them for iteration i; ``keep[c, i]``: margin > MARGIN = 1e-9 and no small curvature
margin pending.  At most 25 % of a case's (start, iteration) pairs and 5 % of the table's may be left out
(LEFT_OUT_CASE, LEFT_OUT_TABLE).

Arithmetic.  ``dtype=np.longdouble`` runs the same replay (values and gradients still float64 functions of the
float64-rounded point) in extended precision.  The largest |U_next_float64 - U_next_longdouble| over the kept steps of the
whole table MAX_CASES, on the trace MaxNumpyDevice makes on the oracle, is the arithmetic noise floor of the
restatement: 2.66e-15 measured (x86 80-bit long double; one step from traced inputs: a few ulp of the unit cube times
the length of a step that the clamp cuts), rounded up to EPS_M = 3e-15 below; tests/test_maximize_cpu.py measures it again on every run and asserts it
stays below EPS_M.  The GPU test allows REPLAY_TOL = 100 x EPS_M = 3e-13: two orders for what the kernel may do
differently at rounding level (its sqrt and division)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONVERGED_G, CONVERGED_F, STALLED, MAXITER, BAD_START, BAD_GRADIENT = range(6)
C1, CURV = 1e-4, 1e-10
EPS_M = 3e-15
REPLAY_TOL = 100 * EPS_M
MARGIN = 1e-9
LEFT_OUT_CASE, LEFT_OUT_TABLE = 0.25, 0.05
MAX_ITER, N_STARTS, MAX_HALVINGS = 6, 16, 12


def _matvec(H, v, free):
    """sum_{j free} H[:, k, j] v[:, j] in the order of j, for free k (0 otherwise)."""
    out = np.zeros_like(v)
    for j in range(v.shape[1]):
        out = out + np.where(free[:, j, None], H[:, :, j] * v[:, j, None], 0.0)
    return np.where(free, out, 0.0)


def _dot(a, b, free):
    out = np.zeros(a.shape[0], dtype=a.dtype)
    for k in range(a.shape[1]):
        out = out + np.where(free[:, k], a[:, k] * b[:, k], 0.0)
    return out


class _Core:
    """The state (u, x, y, g, H) of n starts and the device's steps on it; every method works on a mask of starts."""

    def __init__(self, lo, hi, X0, fixed, H0, max_halvings, gtol, ftol, minus_inf_value, value_of, dtype):
        ft = self.ft = dtype
        self.lo64, self.hi64 = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        self.lo, self.hi = self.lo64.astype(ft), self.hi64.astype(ft)
        self.span = self.hi - self.lo
        X0 = np.asarray(X0, dtype=float)
        self.n, self.d = n, d = X0.shape
        self.fixed = np.asarray(fixed, dtype=bool)
        self.H0 = np.asarray(H0, dtype=float).astype(ft)
        if self.fixed.shape != (d,) or self.H0.shape != (d, d):
            raise ValueError(f"fixed {self.fixed.shape} and H0 {self.H0.shape} do not fit d = {d}")
        self.max_halvings, self.gtol, self.ftol, self.minus_inf = int(max_halvings), float(gtol), float(ftol), minus_inf_value
        self.value_of = value_of
        self.x = X0.astype(ft)
        self.u = (self.x - self.lo) / self.span
        self.y, self.g = np.full(n, np.nan), np.full((n, d), np.nan)
        self.H = np.broadcast_to(self.H0, (n, d, d)).copy()
        self.h0 = np.ones(n, bool)
        self.free = np.zeros((n, d), bool)
        self.prev_free, self.first = np.zeros((n, d), bool), np.ones(n, bool)
        self.ncalls = np.zeros(n, np.int64)
        self.gated_trials = 0

    def reset(self, sel):
        self.H[sel] = self.H0
        self.h0[sel] = True

    def free_set(self, act):
        """Step 1 for the starts in ``act``: (stop, margin) -- the free set is kept in self.free."""
        u, g = self.u, self.g
        wall = ((u == 0) | (u == 1)) & ~self.fixed
        free = ~self.fixed & ~((u == 0) & (g <= 0)) & ~((u == 1) & (g >= 0))
        self.free[act] = free[act]
        with np.errstate(invalid="ignore"):
            gmax = np.max(np.where(free, np.abs(g), 0.0), axis=1)
            m_wall = np.min(np.where(wall, np.abs(g), np.inf), axis=1)
        stop = act & (~free.any(axis=1) | (gmax <= self.gtol))
        m_g = np.where(free.any(axis=1), np.abs(gmax - self.gtol), np.inf)
        return stop, np.minimum(m_wall, m_g)

    def free_change(self, act):
        """Step 2's first rule; returns the resets it made (0 / 1 per start)."""
        ch = act & ~self.first & np.any(self.free != self.prev_free, axis=1) & ~self.h0
        self.reset(ch)
        self.prev_free[act] = self.free[act]
        self.first[act] = False
        return ch.astype(np.int64)

    def search(self, act):
        """Steps 2 and 3 for the starts in ``act``: dict(accepted, stalled, u, x, y, nhalv, nreset, margin)."""
        n, ft = self.n, self.ft
        u, x, y, free = self.u, self.x, self.y, self.free
        g = self.g.astype(ft)
        acc, stalled = np.zeros(n, bool), np.zeros(n, bool)
        nhalv, nreset = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        margin = np.full(n, np.inf)
        ua, xa, ya = u.copy(), x.copy(), np.full(n, np.nan)
        todo = act.copy()
        while todo.any():
            p = _matvec(self.H, g, free)
            pg = _dot(p, g, free)
            with np.errstate(invalid="ignore", divide="ignore"):
                cosine = (pg / np.sqrt(_dot(p, p, free) * _dot(g, g, free))).astype(float)
            margin[todo] = np.minimum(margin[todo], np.abs(np.where(np.isnan(cosine), 0.0, cosine))[todo])
            bad = todo & ~(pg > 0)
            st = bad & self.h0
            stalled |= st
            todo &= ~st
            rs = bad & ~self.h0
            self.reset(rs)
            nreset += rs
            pend = todo & ~rs
            t = ft(1.0)
            for h in range(self.max_halvings + 1):
                if not pend.any():
                    break
                un = np.where(free, np.clip(u + t * p, 0.0, 1.0), u)
                moved = un != u
                xn = np.where(moved, np.where(un == 1, self.hi, np.clip(self.lo + un * self.span, self.lo, self.hi)), x)
                same = pend & ~moved.any(axis=1)
                stalled |= same
                pend &= ~same
                todo &= ~same
                if not pend.any():
                    break
                thr = y + C1 * _dot(g, un - u, free)
                yt = np.full(n, np.nan)
                yt[pend] = self.value_of(np.ascontiguousarray(xn[pend].astype(float)))
                self.ncalls[pend] += 1
                self.gated_trials += int(np.sum(np.isneginf(yt[pend])))
                with np.errstate(invalid="ignore"):
                    ok = pend & np.isfinite(yt) & (yt > self.minus_inf) & (yt >= thr)
                    m = (np.abs(yt - thr) / np.maximum(1.0, np.abs(y))).astype(float)
                m = np.where(pend & np.isfinite(yt), m, np.inf)
                margin = np.minimum(margin, m)
                ua[ok], xa[ok], ya[ok], nhalv[ok] = un[ok], xn[ok], yt[ok], h
                acc |= ok
                pend &= ~ok
                todo &= ~ok
                t = t * ft(0.5)
            st = pend & self.h0
            stalled |= st
            todo &= ~st
            rs = pend & ~self.h0
            self.reset(rs)
            nreset += rs
        return dict(accepted=acc, stalled=stalled, u=ua, x=xa, y=ya, nhalv=nhalv, nreset=nreset, margin=margin)

    def update(self, act, un, gn):
        """Step 5 for the starts in ``act`` with the accepted (u', g'); returns the curvature margin."""
        ft, free = self.ft, self.free
        s = np.where(free, un - self.u, 0.0).astype(ft)
        q = np.where(free, self.g.astype(ft) - np.asarray(gn).astype(ft), 0.0)
        allk = np.ones_like(free)
        Hq = _matvec(self.H, q, free)
        sq, ss, qq, qHq = _dot(s, q, allk), _dot(s, s, allk), _dot(q, q, allk), _dot(q, Hq, allk)
        nrm = np.sqrt(ss * qq)
        with np.errstate(invalid="ignore", divide="ignore"):
            upd = act & (sq > CURV * nrm)
            m = np.where(nrm > 0, np.abs(sq - CURV * nrm) / nrm, np.inf).astype(float)
            rho = 1.0 / sq
            c2 = (rho * rho) * qHq + rho
            Hn = (self.H - rho[:, None, None] * (s[:, :, None] * Hq[:, None, :] + Hq[:, :, None] * s[:, None, :])) \
                + c2[:, None, None] * (s[:, :, None] * s[:, None, :])
        block = upd[:, None, None] & free[:, :, None] & free[:, None, :]
        self.H = np.where(block, Hn, self.H)
        self.h0[upd] = False
        return np.where(act, m, np.inf)

    def converged_f(self, y_old, y_new):
        with np.errstate(invalid="ignore"):
            rhs = self.ftol * np.maximum(1.0, np.abs(y_new))
            stop = (y_new - y_old) <= rhs
            m = np.abs((y_new - y_old) - rhs) if self.ftol > 0 else np.full(len(y_new), np.inf)
        return stop, m


def _check_args(max_iter, max_halvings, gtol, ftol):
    if not 0 <= int(max_iter) <= 100000 or not 0 <= int(max_halvings) <= 1000:
        raise ValueError(f"max_iter = {max_iter}, max_halvings = {max_halvings}")
    if not (np.isfinite(gtol) and gtol >= 0) or not (np.isfinite(ftol) and ftol >= 0):
        raise ValueError(f"gtol = {gtol}, ftol = {ftol}")


class MaxNumpyDevice:
    """``maximize_mean`` of gpry_amd/_lib.py on a numpy log-density and its gradient; keeps the arguments of every call
    in ``calls``."""

    def __init__(self, loglike, grad_x):
        self.loglike, self.grad_x = loglike, grad_x
        self.calls = []
        self.gated_trials = 0          # trial points of all calls that met the gates (-inf)

    def maximize_mean(self, lo, hi, X0, y0, fixed, H0, max_iter, max_halvings, gtol, ftol, minus_inf_value, hooks=False,
                      dtype=np.float64):
        _check_args(max_iter, max_halvings, gtol, ftol)
        max_iter = int(max_iter)
        X0 = np.atleast_2d(np.asarray(X0, dtype=float))
        self.calls.append(dict(X0=X0.copy(), fixed=np.array(fixed, dtype=bool), H0=np.array(H0, dtype=float), max_iter=max_iter))
        co = _Core(lo, hi, X0, fixed, H0, max_halvings, gtol, ftol, minus_inf_value, self.loglike, dtype)
        n, d = co.n, co.d
        span64 = co.hi64 - co.lo64
        grad_u = lambda X: np.asarray(self.grad_x(np.ascontiguousarray(X.astype(float))), dtype=float) * span64  # noqa: E731
        co.y = np.asarray(y0, dtype=float).copy()
        todo = np.isnan(co.y)
        if todo.any():
            co.y[todo] = self.loglike(X0[todo])
            co.ncalls[todo] += 1
        status, iters, ngrad = np.full(n, MAXITER, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        with np.errstate(invalid="ignore"):
            run = np.isfinite(co.y) & (co.y > minus_inf_value) & np.all((co.u >= 0) & (co.u <= 1), axis=1)
        status[~run] = BAD_START
        if run.any():
            co.g[run] = grad_u(co.x[run])
            ngrad[run] += 1
            bad = run & ~np.all(np.isfinite(co.g), axis=1)
            status[bad] = BAD_GRADIENT
            run &= ~bad
        tr = dict(U_tr=np.full((n, max_iter + 1, d), np.nan), y_tr=np.full((n, max_iter + 1), np.nan),
                  G_tr=np.full((n, max_iter + 1, d), np.nan), nhalv_tr=np.full((n, max_iter), -1, np.int32),
                  reset_tr=np.full((n, max_iter), -1, np.int32))
        tr["U_tr"][:, 0], tr["y_tr"][:, 0], tr["G_tr"][:, 0] = co.u.astype(float), co.y, co.g
        while run.any():
            stop, _ = co.free_set(run)
            status[stop] = CONVERGED_G
            run &= ~stop
            status[run & (iters >= max_iter)] = MAXITER
            run &= iters < max_iter
            if not run.any():
                break
            nreset = co.free_change(run)
            r = co.search(run)
            nreset += r["nreset"]
            idx = np.flatnonzero(run)
            tr["nhalv_tr"][idx, iters[idx]], tr["reset_tr"][idx, iters[idx]] = r["nhalv"][idx], nreset[idx]
            status[run & r["stalled"]] = STALLED
            run &= r["accepted"]
            if not run.any():
                break
            gn = np.full((n, d), np.nan)
            gn[run] = grad_u(r["x"][run])
            ngrad[run] += 1
            fin = np.all(np.isfinite(gn), axis=1)
            co.update(run & fin, r["u"], gn)
            y_old = co.y.copy()
            co.u[run], co.x[run], co.y[run], co.g[run] = r["u"][run], r["x"][run], r["y"][run], gn[run]
            iters[run] += 1
            idx = np.flatnonzero(run)
            tr["U_tr"][idx, iters[idx]], tr["y_tr"][idx, iters[idx]], tr["G_tr"][idx, iters[idx]] = \
                co.u[idx].astype(float), co.y[idx], co.g[idx]
            status[run & ~fin] = BAD_GRADIENT
            run &= fin
            cf = run & co.converged_f(y_old, co.y)[0]
            status[cf] = CONVERGED_F
            run &= ~cf
        self.gated_trials += co.gated_trials
        out = dict(X=co.x.astype(float), y=co.y.copy(), G=co.g.copy(), iters=iters, ncalls=co.ncalls.copy(), ngrad=ngrad,
                   status=status, device_ms=0.0)
        if hooks:
            out.update(tr)
        return out


def replay(trace, lo, hi, X0, fixed, H0, max_iter, max_halvings, gtol, ftol, minus_inf_value, value_of, dtype=np.float64):
    """See the module's docstring."""
    U, G, Y = trace["U_tr"], trace["G_tr"], trace["y_tr"]
    co = _Core(lo, hi, X0, fixed, H0, max_halvings, gtol, ftol, minus_inf_value, value_of, dtype)
    n, d, ft = co.n, co.d, dtype
    max_iter = int(max_iter)
    out = dict(U_next=np.full((n, max_iter, d), np.nan), nhalv=np.full((n, max_iter), -1, np.int64),
               reset=np.full((n, max_iter), -1, np.int64), ran=np.zeros((n, max_iter), bool),
               margin=np.full((n, max_iter + 1), np.inf), keep=np.zeros((n, max_iter + 1), bool),
               end_iters=np.full(n, -1, np.int64), end_status=np.full(n, -1, np.int64))
    started = np.all(np.isfinite(G[:, 0]), axis=1)         # (BAD_START / BAD_GRADIENT at the start: nothing to replay)
    ended = ~started
    tainted = np.zeros(n, bool)                            # a small curvature margin since the last reset of H
    for i in range(max_iter + 1):
        have = ~ended & ~np.isnan(Y[:, i])
        if not have.any():
            break
        co.u[have], co.y[have], co.g[have] = U[have, i].astype(ft), Y[have, i], G[have, i]
        if i > 0:
            moved = U[:, i] != U[:, i - 1]
            xn = np.where(co.u == 1, co.hi, np.clip(co.lo + co.u * co.span, co.lo, co.hi))
            co.x = np.where(have[:, None] & moved, xn, co.x)
        stop, m = co.free_set(have)
        out["margin"][have, i] = m[have]
        last = have & ~stop & (i >= max_iter)
        for sel, code in ((stop, CONVERGED_G), (last, MAXITER)):
            out["end_iters"][sel], out["end_status"][sel] = i, code
        ended |= stop | last
        act = have & ~stop & ~last
        if i < max_iter and act.any():
            nreset = co.free_change(act)
            r = co.search(act)
            nreset += r["nreset"]
            tainted &= co.h0 == 0
            out["U_next"][act, i], out["nhalv"][act, i], out["reset"][act, i] = r["u"][act].astype(float), r["nhalv"][act], nreset[act]
            out["ran"][act, i] = True
            out["margin"][act, i] = np.minimum(out["margin"][act, i], r["margin"][act])
            st = act & r["stalled"]
            out["end_iters"][st], out["end_status"][st] = i, STALLED
            ended |= st
            # the history goes on with the trace's own iterate i + 1, and its resets
            nxt = act & ~np.isnan(Y[:, i + 1])
            co.reset(nxt & (trace["reset_tr"][:, i] > 0) & ~co.h0)
            gn = G[:, i + 1]
            fin = np.all(np.isfinite(gn), axis=1)
            mc = co.update(nxt & fin, U[:, i + 1].astype(ft), gn)
            bg = nxt & ~fin
            out["end_iters"][bg], out["end_status"][bg] = i + 1, BAD_GRADIENT
            cf, mf = co.converged_f(Y[:, i], Y[:, i + 1])
            cf = nxt & fin & cf
            out["margin"][nxt & fin, i] = np.minimum(out["margin"][nxt & fin, i], mf[nxt & fin])
            out["end_iters"][cf], out["end_status"][cf] = i + 1, CONVERGED_F
            ended |= bg | cf | (act & ~nxt)
            out["keep"][have, i] = (out["margin"][have, i] > MARGIN) & ~tainted[have]
            tainted |= nxt & (mc <= MARGIN)
        else:
            out["keep"][have, i] = (out["margin"][have, i] > MARGIN) & ~tainted[have]
    return out


def trace_points(trace, lo, hi, X0):
    """The raw points (nstart, max_iter + 1, d) of the traced iterates, by the device's rule: a coordinate whose u did
    not change keeps its x, one that did is clamp(lo + u (hi - lo)), hi itself at u = 1.  NaN in unused slots."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    U = trace["U_tr"]
    X = np.full(U.shape, np.nan)
    X[:, 0] = X0
    for i in range(1, U.shape[1]):
        xn = np.where(U[:, i] == 1, hi, np.clip(lo + U[:, i] * (hi - lo), lo, hi))
        X[:, i] = np.where(U[:, i] != U[:, i - 1], xn, X[:, i - 1])
        X[np.isnan(trace["y_tr"][:, i]), i] = np.nan
    return X


def left_out(rep):
    """(left out, all) (start, iteration) pairs whose search the replay ran."""
    return int(np.sum(rep["ran"] & ~rep["keep"][:, :-1])), int(np.sum(rep["ran"]))


# ---- the walk table -------------------------------------------------------------------------------------------------
def _cases():
    import sampler_walk as sw
    c = {}
    # d in {1, 3, 5, 9, 17, 32} x N in {70, 1100, 2500}, the four kernels, affine on and off, the masks
    c["d=1 RBF N=70"] = dict(model=dict(d=1, kid=sw.RBF, N=70, affine=True))
    c["d=3 M52 N=1100 one fixed"] = dict(model=dict(d=3, kid=sw.M52, N=1100, affine=False), fixed=[1])
    c["d=5 M12 N=70 two fixed"] = dict(model=dict(d=5, kid=sw.M12, N=70, affine=True), fixed=[0, 3])
    c["d=9 M32 N=1100"] = dict(model=dict(d=9, kid=sw.M32, N=1100, affine=False))
    c["d=17 RBF N=2500"] = dict(model=dict(d=17, kid=sw.RBF, N=2500, affine=True))
    c["d=32 M52 N=1100"] = dict(model=dict(d=32, kid=sw.M52, N=1100, affine=False))
    c["d=5 M32 N=2500 all but one fixed"] = dict(model=dict(d=5, kid=sw.M32, N=2500, affine=False), fixed=[0, 1, 3, 4])
    c["d=9 M12 N=1100"] = dict(model=dict(d=9, kid=sw.M12, N=1100, affine=True))
    # the box's wall cuts the peak (at 0.3) off: the free set shrinks on the way and H is reset
    c["wall cuts the peak"] = dict(model=dict(d=3, kid=sw.M52, N=1100, affine=True), hi={0: -0.2, 2: 0.1})
    c["starts on walls and corners"] = dict(model=dict(d=3, kid=sw.RBF, N=600, affine=False), walls=True)
    # SVM + trust region (tests/test_nested_gpu.py: _svm_model): a long first step lands on gated ground
    c["gated"] = dict(model=dict(d=3, kid=sw.M52, N=300, svm=True, seed=9), h0_scale=8.0)
    return c


class Walk:
    """The inputs of one ``maximize_mean`` call of a case, made from the oracle alone, so that the CPU and the GPU file
    run the same searches.  Model: that of ``hmc_numpy.Walk`` (normalize_y off, noise 0.1).  Starts: N_STARTS training
    rows from the upper part of the ranking but away from the best, so that the search and not rounding decides.  H0:
    maximize_gp's (the weighted covariance of the training set in the unit cube, ridged)."""

    def __init__(self, name, gpr_device=None):
        import sampler_walk as sw
        from hmc_numpy import oracle_grad_x
        from gpry_amd.mcmc import _weighted_cov
        from gpry_amd.nested import cholesky_ridged
        case = _cases()[name]
        margs = dict(case["model"])
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
        for k, v in case.get("hi", {}).items():
            self.hi[k] = v
        X, y = (self.gpr.X_train, self.gpr.y_train) if m.svm else (m.X, m.y)
        ok = np.all((X >= self.lo) & (X <= self.hi), axis=1) & np.isfinite(y)
        X, y = X[ok], y[ok]
        order = np.argsort(-y, kind="stable")
        first = max(4, len(order) // 20)
        self.X0 = np.ascontiguousarray(X[order[first:first + 3 * N_STARTS:3]])
        assert len(self.X0) == N_STARTS, (name, len(self.X0))
        if case.get("walls"):
            # the box drawn in to the starts' own extent, then every start put on one to three walls
            self.lo, self.hi = self.X0.min(axis=0) - 0.05, self.X0.max(axis=0) + 0.05
            rng = np.random.default_rng(4)
            for r in range(N_STARTS):
                ks = rng.choice(d, size=1 + r % d, replace=False)
                self.X0[r, ks] = np.where(rng.random(len(ks)) < 0.5, self.lo[ks], self.hi[ks])
        span = self.hi - self.lo
        self.fixed = np.zeros(d, bool)
        self.fixed[case.get("fixed", [])] = True
        L = cholesky_ridged(_weighted_cov(X, y) / np.outer(span, span))
        self.H0 = case.get("h0_scale", 1.0) * (L @ L.T)
        # (gtol in the unit cube: the ascents of the low dimensions end before their steps reach the rounding of y)
        self.gtol, self.ftol, self.minus_inf_value = 1e-3, 0.0, -np.inf

    def args(self):
        return (self.lo, self.hi, self.X0, np.full(len(self.X0), np.nan), self.fixed, self.H0, MAX_ITER, MAX_HALVINGS,
                self.gtol, self.ftol, self.minus_inf_value)

    def trace(self):
        """The oracle-side trace: ``MaxNumpyDevice`` with the hooks."""
        return MaxNumpyDevice(self.loglike, self.grad_x).maximize_mean(*self.args(), hooks=True)

    def replay(self, trace, value_of=None, dtype=np.float64):
        return replay(trace, self.lo, self.hi, self.X0, self.fixed, self.H0, MAX_ITER, MAX_HALVINGS, self.gtol, self.ftol,
                      self.minus_inf_value, value_of if value_of is not None else self.loglike, dtype)


MAX_CASES = list(_cases())


# ---- the host code on a stand-in ------------------------------------------------------------------------------------
class HostGpr:
    """What ``maximize_gp`` / ``profile_gp`` need of a regressor, around a stand-in device."""

    def __init__(self, device, X, y, bounds, minus_inf_value=-np.inf):
        self.device, self.X_train, self.y_train = device, np.asarray(X, dtype=float), np.asarray(y, dtype=float)
        self.bounds, self.trust_bounds, self.minus_inf_value, self.n_eval = np.asarray(bounds, dtype=float), None, minus_inf_value, 0

    def _ensure_factor(self):
        pass

    _push_affine = _ensure_factor

    def _push_gates(self):
        return True


# the end-to-end models (tests/test_maximize_gpu.py): name -> arguments of sampler_walk.Model
E2E_MODELS = {"d=2": dict(d=2, kid=3, N=300, seed=3), "d=3": dict(d=3, kid=3, N=500, seed=5)}
E2E_GRID_1D = np.linspace(-1.2, 1.6, 9)
E2E_GRID_2D = np.array([[a, b] for a in (-0.5, 0.3, 1.0) for b in (-0.4, 0.3, 0.9)])


def e2e_oracle(name, perturb=0.0):
    """(model, oracle-side HostGpr) of an end-to-end model; ``perturb``: the size of a random shift of the training
    rows the starts are taken from (the oracle itself keeps the rows as they are)."""
    import sampler_walk as sw
    from hmc_numpy import oracle_grad_x
    m = sw.Model(**E2E_MODELS[name])
    ref = m.oracle()
    mean = m.mean_fn(ref)
    clip = float(ref.clip_hi())
    dev = MaxNumpyDevice(lambda X: np.minimum(mean(X), clip), oracle_grad_x(ref))
    X = m.X + perturb * np.random.default_rng(1).uniform(-1, 1, m.X.shape)
    return m, HostGpr(dev, np.clip(X, m.bounds[:, 0], m.bounds[:, 1]), m.y, m.bounds)


def e2e_results(gpr, d):
    """The three end-to-end results of a regressor (real or stand-in): best y, 1-D profile, 2-D profile."""
    from gpry_amd.maximize import maximize_gp, profile_gp
    r = maximize_gp(gpr, nstarts=32)
    p1 = profile_gp(gpr, 0, E2E_GRID_1D, nstarts=8)
    p2 = profile_gp(gpr, (0, d - 1), E2E_GRID_2D, nstarts=8)
    return r, p1, p2
