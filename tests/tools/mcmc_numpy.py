"""numpy stand-in for the device call of gpry_amd/mcmc.py (``dev.mcmc_chains``, kernel in gpry_amd/csrc/mcmc.hip), and
the restatement of one Metropolis step the GPU tests check the kernel against.

``NumpyMCMCDevice(loglike)``: the device's algorithm on a numpy log-likelihood ``loglike(X (m, d)) -> (m,)`` -- the same
Philox counters (phase 3, draw j, batch, chain, step), the same box test and acceptance rule, chains vectorised,
Box-Muller and the proposal product in numpy: the same distribution as the device, not the same bits."""
import numpy as np

from ns_philox import philox

PHASE_MCMC, DRAW_ACCEPT = 3, 16


def normals(seed, batch, chains, step, d):
    """z (len(chains), d) of step ``step``: Box-Muller of draws 0..(d-1)/2, as the kernel does."""
    h = (d + 1) // 2
    chains = np.asarray(chains)
    ua, ub = philox(seed, PHASE_MCMC, np.arange(h)[None, :], batch, chains[:, None], step)
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - ua)), 2 * np.pi * ub
    z = np.empty((len(chains), 2 * h))
    z[:, 0::2], z[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
    return z[:, :d]


def accept_uniform(seed, batch, chains, step):
    return philox(seed, PHASE_MCMC, DRAW_ACCEPT, batch, np.asarray(chains), step)[0]


class NumpyMCMCDevice:
    """``mcmc_chains`` of gpry_amd/_lib.py on a numpy log-likelihood; keeps the arguments of every call in ``calls``."""

    def __init__(self, loglike):
        self.loglike = loglike
        self.calls = []

    def mcmc_chains(self, lo, hi, X0, y0, Lp, T, minus_inf_value, seed, batch, nsteps, thin, proposals=False):
        lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        span = hi - lo
        X0 = np.asarray(X0, dtype=float)
        n, d = X0.shape
        if not (T > 0 and np.isfinite(T)):
            raise ValueError(f"temperature T = {T}")
        self.calls.append(dict(batch=batch, nsteps=nsteps, thin=thin, Lp=np.array(Lp), T=T, nchains=n))
        c = np.arange(n)
        x = X0.copy()
        u = (x - lo) / span
        y = np.asarray(y0, dtype=float).copy()
        cnt = np.zeros(n, np.int64)
        nacc = np.zeros(n, np.int64)
        todo = np.isnan(y)
        if todo.any():
            y[todo] = self.loglike(x[todo])
            cnt[todo] += 1
        nrec = nsteps // thin
        Xr, yr = np.empty((n, nrec, d)), np.empty((n, nrec))
        Xprop, yprop = np.empty((n, nsteps, d)), np.empty((n, nsteps))
        for s in range(nsteps):
            ut = u + normals(seed, batch, c, s, d) @ np.asarray(Lp).T
            xt = lo + ut * span
            inside = np.all((ut >= 0) & (ut <= 1) & (xt >= lo) & (xt <= hi), axis=1)
            yt = np.full(n, np.nan)
            if inside.any():
                yt[inside] = self.loglike(xt[inside])
                cnt[inside] += 1
            Xprop[:, s], yprop[:, s] = xt, yt
            ua = accept_uniform(seed, batch, c, s)
            with np.errstate(invalid="ignore"):
                acc = inside & np.isfinite(yt) & (yt > minus_inf_value) & (np.log(1.0 - ua) < (yt - y) / T)
            x[acc], u[acc], y[acc] = xt[acc], ut[acc], yt[acc]
            nacc += acc
            if (s + 1) % thin == 0:
                Xr[:, (s + 1) // thin - 1], yr[:, (s + 1) // thin - 1] = x, y
        out = dict(X=Xr, y=yr, X_last=x, y_last=y, naccept=nacc, ncalls=cnt, device_ms=0.0)
        if proposals:
            out.update(X_prop=Xprop, y_prop=yprop)
        return out
