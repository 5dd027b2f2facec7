"""numpy restatement of the draws of gpry_amd/csrc/nested.hip, and a numpy stand-in for the two device calls of
gpry_amd/nested.py.

``philox(seed, phase, draw, gen, chain, step)``: Philox4x32-10 of the counter (phase << 24 | draw, gen, chain, step)
under the key (seed mod 2^32, seed >> 32), as two uniforms in [0, 1) with 53 bits each -- the device's ns_philox,
vectorised over any argument.  ``prior_points`` is the device's prior draw bit for bit.

``NumpyNestedDevice(loglike)``: ``ns_prior`` / ``ns_generation`` with the device's algorithm (the same counters, the
same stepping-out and shrinkage caps), chains vectorised, Box-Muller in numpy -- the same distribution as the device, not
the same bits."""
import numpy as np

PHASE_PRIOR, PHASE_START, PHASE_STEP = 0, 1, 2
DRAW_OFFSET, DRAW_SHRINK = 16, 17
STEP_OUT_MAX, SHRINK_MAX = 32, 64
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def philox(seed, phase, draw, gen, chain, step):
    seed = int(seed)
    b = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (phase, draw, gen, chain, step)))
    phase, draw, gen, chain, step = b
    c0 = ((phase << np.uint64(24)) | draw) & _MASK
    c1, c2, c3 = gen & _MASK, chain & _MASK, step & _MASK
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    a = (((c0 << np.uint64(32)) | c1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    b_ = (((c2 << np.uint64(32)) | c3) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return a, b_


def prior_points(lo, hi, seed, n):
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    d = len(lo)
    i = np.arange(n)[:, None]
    k = np.arange(d)[None, :]
    ua, ub = philox(seed, PHASE_PRIOR, k // 2, 0, i, 0)
    u = np.where(k % 2 == 1, ub, ua)
    return np.minimum(lo + u * (hi - lo), hi)


class NumpyNestedDevice:
    """The two calls of gpry_amd/nested.py on a numpy log-likelihood ``loglike(X (m, d)) -> (m,)``."""

    def __init__(self, loglike):
        self.loglike = loglike
        self.calls = []

    def ns_prior(self, lo, hi, seed, n):
        X = prior_points(lo, hi, seed, n)
        return X, np.asarray(self.loglike(X), dtype=float), 0.0

    def ns_generation(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats):
        """``W``: lower triangular (the kernel sums k <= t only; what lies above the diagonal is not read)."""
        lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        span = hi - lo
        n, d = X_surv.shape
        self.calls.append(dict(generation=generation, k=k, lstar=lstar, nsurv=n))
        c = np.arange(k)
        us, _ = philox(seed, PHASE_START, 0, generation, c, 0)
        j = np.minimum((us * n).astype(np.int64), n - 1)
        x = X_surv[j].copy()
        y = np.asarray(y_surv, dtype=float)[j].copy()
        u = (x - lo) / span
        cnt = np.zeros(k, dtype=np.int64)

        def attempt(t, v, act):
            """(accepted, y) of the points u + t v of the chains in `act`."""
            ut = u + t[:, None] * v
            xt = lo + ut * span
            inside = act & np.all((ut >= 0) & (ut <= 1) & (xt >= lo) & (xt <= hi), axis=1)
            yt = np.full(k, -np.inf)
            if inside.any():
                yt[inside] = self.loglike(xt[inside])
                cnt[inside] += 1
            return inside & (yt > lstar), yt, ut, xt

        h = (d + 1) // 2
        for s in range(num_repeats):
            ua, ub = philox(seed, PHASE_STEP, np.arange(h)[None, :], generation, c[:, None], s)
            rad, ang = np.sqrt(-2.0 * np.log(1.0 - ua)), 2 * np.pi * ub
            z = np.empty((k, 2 * h))
            z[:, 0::2], z[:, 1::2] = rad * np.cos(ang), rad * np.sin(ang)
            z = z[:, :d]
            v = z @ np.tril(np.asarray(W)).T / np.linalg.norm(z, axis=1)[:, None]
            r, _ = philox(seed, PHASE_STEP, DRAW_OFFSET, generation, c, s)
            lt, rt = -r, 1.0 - r
            act = np.ones(k, bool)
            for _ in range(STEP_OUT_MAX):
                ok = attempt(lt, v, act)[0]
                lt = np.where(ok, lt - 1.0, lt)
                act = ok
                if not act.any():
                    break
            act = np.ones(k, bool)
            for _ in range(STEP_OUT_MAX):
                ok = attempt(rt, v, act)[0]
                rt = np.where(ok, rt + 1.0, rt)
                act = ok
                if not act.any():
                    break
            todo = np.ones(k, bool)
            for q in range(SHRINK_MAX):
                w, _ = philox(seed, PHASE_STEP, DRAW_SHRINK + q, generation, c, s)
                t = lt + w * (rt - lt)
                ok, yt, ut, xt = attempt(t, v, todo)
                u[ok], x[ok], y[ok] = ut[ok], xt[ok], yt[ok]
                miss = todo & ~ok
                lt = np.where(miss & (t < 0), t, lt)
                rt = np.where(miss & (t >= 0), t, rt)
                todo = miss
                if not todo.any():
                    break
        return x, y, cnt, 0.0
