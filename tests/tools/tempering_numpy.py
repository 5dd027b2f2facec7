"""numpy stand-in for the device call of gpry_amd/tempering.py (``dev.mcmc_ladders``, kernel in
gpry_amd/csrc/mcmc_ladders.hip).

``NumpyLadderDevice(loglike)``: the device's algorithm on a numpy log-likelihood ``loglike(X (m, d)) -> (m,)`` -- slot r
of ladder a is chain c = a nrungs + r and makes the Metropolis step of ``mcmc_numpy.NumpyMCMCDevice`` with Lp[r] and T[r]
(the same Philox counters, box test and acceptance rule); after every ``swap_every``-th step the swap round of the kernel:
round q = (s + 1) / swap_every - 1, pairs (r, r + 1) with r = q (mod 2), tried iff both y are usable, uniform = draw 17 of
chain c_r at step s, accepted iff log(1 - us) < (1 / T[r] - 1 / T[r + 1]) (y_{r+1} - y_r).  The same distribution as
the device, not the same bits."""
import numpy as np

from mcmc_numpy import PHASE_MCMC, accept_uniform, normals
from ns_philox import philox

DRAW_SWAP = 17


def swap_uniform(seed, batch, chains, step):
    return philox(seed, PHASE_MCMC, DRAW_SWAP, batch, np.asarray(chains), step)[0]


class NumpyLadderDevice:
    """``mcmc_ladders`` of gpry_amd/_lib.py on a numpy log-likelihood; keeps the arguments of every call in ``calls``."""

    def __init__(self, loglike):
        self.loglike = loglike
        self.calls = []

    def mcmc_ladders(self, lo, hi, X0, y0, nrungs, Lp, T, minus_inf_value, seed, batch, nsteps, thin, swap_every,
                     proposals=False):
        lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        span = hi - lo
        X0 = np.asarray(X0, dtype=float)
        n, d = X0.shape
        R = int(nrungs)
        Lp, T = np.asarray(Lp, dtype=float).reshape(R, d, d), np.asarray(T, dtype=float).reshape(R)
        if not 1 <= R <= 8 or n % R:
            raise ValueError(f"{n} chains do not form ladders of nrungs = {R} (1 .. 8)")
        if not np.all((T > 0) & np.isfinite(T)):
            raise ValueError(f"temperatures T = {T}")
        if swap_every < 0:
            raise ValueError(f"swap_every = {swap_every}")
        nl = n // R
        self.calls.append(dict(batch=batch, nsteps=nsteps, thin=thin, Lp=Lp.copy(), T=T.copy(), nchains=n, nrungs=R,
                               swap_every=swap_every))
        c = np.arange(n)
        rung = c % R
        Tc = T[rung]
        x = X0.copy()
        u = (x - lo) / span
        y = np.asarray(y0, dtype=float).copy()
        cnt, nacc = np.zeros(n, np.int64), np.zeros(n, np.int64)
        ntry, nsw = np.zeros((nl, R - 1), np.int64), np.zeros((nl, R - 1), np.int64)
        todo = np.isnan(y)
        if todo.any():
            y[todo] = self.loglike(x[todo])
            cnt[todo] += 1
        nrec = nsteps // thin
        nround = nsteps // swap_every if swap_every > 0 else 0
        Xr, yr = np.empty((n, nrec, d)), np.empty((n, nrec))
        Xprop, yprop = np.empty((n, nsteps, d)), np.empty((n, nsteps))
        log = np.full((nl, nround, R - 1), -1, np.int8)
        for s in range(nsteps):
            z = normals(seed, batch, c, s, d)
            ut = u.copy()
            for r in range(R):
                ut[rung == r] += z[rung == r] @ Lp[r].T
            xt = lo + ut * span
            inside = np.all((ut >= 0) & (ut <= 1) & (xt >= lo) & (xt <= hi), axis=1)
            yt = np.full(n, np.nan)
            if inside.any():
                yt[inside] = self.loglike(xt[inside])
                cnt[inside] += 1
            Xprop[:, s], yprop[:, s] = xt, yt
            ua = accept_uniform(seed, batch, c, s)
            with np.errstate(invalid="ignore"):
                acc = inside & np.isfinite(yt) & (yt > minus_inf_value) & (np.log(1.0 - ua) < (yt - y) / Tc)
            x[acc], u[acc], y[acc] = xt[acc], ut[acc], yt[acc]
            nacc += acc
            if swap_every > 0 and (s + 1) % swap_every == 0:
                q = (s + 1) // swap_every - 1
                for r in range(q % 2, R - 1, 2):
                    a, b = np.arange(nl) * R + r, np.arange(nl) * R + r + 1
                    with np.errstate(invalid="ignore"):
                        tried = (np.isfinite(y[a]) & (y[a] > minus_inf_value) & np.isfinite(y[b])
                                 & (y[b] > minus_inf_value))
                        us = swap_uniform(seed, batch, a, s)
                        sw = tried & (np.log(1.0 - us) < (1.0 / T[r] - 1.0 / T[r + 1]) * (y[b] - y[a]))
                    ntry[:, r] += tried
                    nsw[:, r] += sw
                    log[:, q, r] = np.where(tried, sw.astype(np.int8), -1)
                    ia, ib = a[sw], b[sw]
                    for arr in (x, u, y):
                        arr[ia], arr[ib] = arr[ib].copy(), arr[ia].copy()
            if (s + 1) % thin == 0:
                Xr[:, (s + 1) // thin - 1], yr[:, (s + 1) // thin - 1] = x, y
        out = dict(X=Xr, y=yr, X_last=x, y_last=y, naccept=nacc, ncalls=cnt, nswap_try=ntry, nswap_acc=nsw,
                   device_ms=0.0)
        if proposals:
            out.update(X_prop=Xprop, y_prop=yprop, swap_log=log)
        return out
