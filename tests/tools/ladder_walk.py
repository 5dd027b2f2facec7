"""Step-by-step host restatement of the tempered ladders' walk (gpry_amd/csrc/mcmc_ladders.hip): every Metropolis decision as
``sampler_walk.check_metropolis_rule`` restates it for the plain chains, and every swap round."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcmc_numpy  # noqa: E402
from tempering_numpy import swap_uniform  # noqa: E402


def check_ladder_rule(dev, lo, hi, X0, y0, y_start, nrungs, Lp, T, minus_inf_value, seed, batch, steps, thin, swap_every):
    """Runs ``dev.mcmc_ladders(..., proposals=True)`` and checks every step against the rule restated with the numpy
    Philox draws.  Metropolis, slot r with Lp[r] and T[r]: the proposal is the previous state + (z Lp[r]^T) span to 1e-13
    max|bounds|; it is evaluated iff it lies in the box; the step is accepted iff y' is finite, above minus_inf_value and
    log(1 - ua) < (y' - y) / T[r].  Swap round q after step s, (s + 1) % swap_every == 0: only the pairs (r, r + 1) with
    r = q (mod 2) appear in the log; a pair is tried iff both current y are finite and above minus_inf_value; it is
    accepted iff log(1 - us) < (1 / T[r] - 1 / T[r + 1]) (y_{r+1} - y_r), us = draw 17 of chain c_r at step s.  Decisions
    within 1e-12 (1 + |rhs|) of their threshold are left out (fewer than 3 in all): after a borderline Metropolis step the
    chain, and whatever it swaps with, is no longer compared; a borderline swap is taken as the device took it.  The
    states are exchanged as the log says, and the records, the final states, naccept, ncalls and nswap_try / nswap_acc
    follow.  ``y0``: what the call is given (NaN: the kernel evaluates the start); ``y_start``: the y the rule starts
    from.  Returns a dict of counts."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    span = hi - lo
    n, d = X0.shape
    R = int(nrungs)
    nl = n // R
    T = np.asarray(T, dtype=float)
    out = dev.mcmc_ladders(lo, hi, X0, y0, R, Lp, T, minus_inf_value, seed, batch, steps, thin, swap_every, proposals=True)
    c = np.arange(n)
    rung = c % R
    Tc = T[rung]
    LT = np.array([np.tril(L).T for L in np.asarray(Lp, dtype=float)])
    X_prev, y_prev = np.array(X0, dtype=float), np.array(y_start, dtype=float)
    tainted = np.zeros(n, bool)
    naccept = np.zeros(n, np.int64)
    ntry, nsw = np.zeros((nl, R - 1), np.int64), np.zeros((nl, R - 1), np.int64)
    outside = borderline = 0
    parities = set()
    atol = 1e-13 * max(np.max(np.abs(lo)), np.max(np.abs(hi)))
    log = out["swap_log"]
    assert log.shape == (nl, steps // swap_every if swap_every > 0 else 0, R - 1)
    for s in range(steps):
        z = mcmc_numpy.normals(seed, batch, c, s, d)
        Xp, yp = out["X_prop"][:, s], out["y_prop"][:, s]
        ok = ~tainted
        step = np.einsum("cj,cjk->ck", z, LT[rung]) * span
        np.testing.assert_allclose((Xp - X_prev)[ok], step[ok], rtol=0, atol=atol)
        inside = np.all((Xp >= lo) & (Xp <= hi), axis=1)
        np.testing.assert_array_equal(np.isnan(yp), ~inside)
        outside += int(np.sum(~inside))
        lu = np.log(1.0 - mcmc_numpy.accept_uniform(seed, batch, c, s))
        with np.errstate(invalid="ignore"):
            rhs = (yp - y_prev) / Tc
            expect = inside & np.isfinite(yp) & (yp > minus_inf_value) & (lu < rhs)
            close = inside & (np.abs(lu - rhs) < 1e-12 * (1 + np.abs(rhs)))
        borderline += int(np.sum(close & ok))
        tainted |= close
        X_prev = np.where(expect[:, None], Xp, X_prev)
        y_prev = np.where(expect, yp, y_prev)
        naccept += expect
        if swap_every > 0 and (s + 1) % swap_every == 0:
            q = (s + 1) // swap_every - 1
            parities.add(q % 2)
            for r in range(R - 1):
                lg = log[:, q, r]
                if r % 2 != q % 2:
                    assert np.all(lg == -1), (s, r)
                    continue
                a, b = np.arange(nl) * R + r, np.arange(nl) * R + r + 1
                ok = ~tainted[a] & ~tainted[b]
                ya, yb = y_prev[a], y_prev[b]
                tried = np.isfinite(ya) & (ya > minus_inf_value) & np.isfinite(yb) & (yb > minus_inf_value)
                lhs = np.log(1.0 - swap_uniform(seed, batch, a, s))
                with np.errstate(invalid="ignore"):
                    rhs = (1.0 / T[r] - 1.0 / T[r + 1]) * (yb - ya)
                    close = tried & (np.abs(lhs - rhs) < 1e-12 * (1 + np.abs(rhs)))
                    expect = tried & (lhs < rhs)
                np.testing.assert_array_equal((lg >= 0)[ok], tried[ok])
                sure = ok & ~close
                np.testing.assert_array_equal((lg == 1)[sure], expect[sure])
                borderline += int(np.sum(close & ok))
                ntry[:, r] += lg >= 0
                nsw[:, r] += lg == 1
                ia, ib = a[lg == 1], b[lg == 1]             # the states change places as the log says
                X_prev[ia], X_prev[ib] = X_prev[ib].copy(), X_prev[ia].copy()
                y_prev[ia], y_prev[ib] = y_prev[ib].copy(), y_prev[ia].copy()
                tainted[ia], tainted[ib] = tainted[ib].copy(), tainted[ia].copy()
        if (s + 1) % thin == 0:
            k = (s + 1) // thin - 1
            ok = ~tainted
            np.testing.assert_array_equal(out["X"][:, k][ok], X_prev[ok])
            np.testing.assert_array_equal(out["y"][:, k][ok], y_prev[ok])
    assert borderline < 3
    assert out["X"].shape == (n, steps // thin, d)
    ok = ~tainted
    np.testing.assert_array_equal(out["X_last"][ok], X_prev[ok])
    np.testing.assert_array_equal(out["y_last"][ok], y_prev[ok])
    if not tainted.any():
        np.testing.assert_array_equal(out["naccept"], naccept)
    np.testing.assert_array_equal(out["ncalls"], np.isnan(y0).astype(np.int64) + np.sum(~np.isnan(out["y_prop"]), axis=1))
    np.testing.assert_array_equal(out["nswap_try"], ntry)
    np.testing.assert_array_equal(out["nswap_acc"], nsw)
    return dict(outside=outside, borderline=borderline, accepted=int(out["naccept"].sum()), parities=parities,
                swaps_accepted=int(np.sum(log == 1)), swaps_rejected=int(np.sum(log == 0)), out=out)
