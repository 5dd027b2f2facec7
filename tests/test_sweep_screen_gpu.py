"""The FP32 screen of the bound pass (option "sweep_screen"): with the screen on and off, on the same context, stage A leaves
the same bounds bit for bit, skips the same blocks and ends in the same shortlists and arrays -- the full sweep's.  The pools
hold what the screen must not get wrong: far candidates (certified), candidates on and next to training rows (live), rows
beyond uhi (live), a NaN, an inf and a coordinate beyond FP32 range (their wave never screens), and, in a wave of their own
that does screen, pairs placed within a few delta of ubnd on both sides (the fall-through to the FP64 test).  What the rows
beyond uhi and the pairs around ubnd do is counted against the same pool without them."""
import functools
import os
import sys
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCALE = {0: 0.5, 2: 3.0, 3: 5.0}
# N: one ragged row chunk, two chunks, padding rows; d: every DP specialisation (4, 4, 8, 16, 24, 32); M and sweep_chunk: a
# ragged candidate tail, several chunks; every kernel id that takes the bound pass; with and without a mask
# (the model of a case with d <= 3 has every length scale at 1e-3 of the box: _case)
#        N    d   M     chunk  kid mask
CASES = ((17, 1, 129, 1024, 0, False),
         (129, 3, 600, 1024, 2, True),
         (257, 5, 5000, 1024, 3, False),
         (129, 16, 5000, 32768, 3, True),
         (257, 21, 600, 32768, 3, False),     # (not RBF: at d = 21 most rows of such a model lie beyond its uhi = 1e6 of each other)
         (257, 32, 5000, 1024, 2, False),
         (17, 16, 5000, 32768, 2, True),
         (257, 16, 600, 1024, 2, True),       # (nor at d = 16)
         (129, 5, 5000, 32768, 0, False))
INFO_KEYS = ("live_blocks", "blocks", "y_bound", "survivors", "rounds", "contracted")


def _corr(kid, u):
    t = np.sqrt(u)
    return np.exp(-u) if kid == 0 else (1.0 + t) * np.exp(-t) if kid == 2 else (1.0 + t + t * t / 3.0) * np.exp(-t)


def _ubnd(kid, C, a1):
    """The bound pass's threshold (sweep.hip: mean_bound_setup), to the accuracy of its own bisection."""
    scale, target = 2.0 * C * a1, 1e-13
    lo, hi = 100.0 * SCALE[kid], 1e6 if kid == 0 else 1e12
    if scale * _corr(kid, lo) <= target:
        return lo
    for _ in range(200):
        if hi <= lo * (1.0 + 1e-9):
            break
        mid = np.sqrt(lo * hi)
        if scale * _corr(kid, mid) <= target:
            hi = mid
        else:
            lo = mid
    return hi


S_NEAR = (0.1, 0.25, 0.5)          # u = ubnd + s delta with the wave's own delta: the FP64 test skips, the screen must not certify
S_FAR = (2.0, 10.0, 100.0)         # ... beyond the margin: either test may skip
S_BELOW = (-0.1, -0.5, -1.0, -2.0, -10.0, -100.0)      # ... below ubnd: live


def _u_all(m, bounds, X, kid, Xc):
    """u of every (training row and one zero padding row, candidate) pair from the coordinates, and both sides' norms."""
    lo, span, ls = bounds[:, 0], bounds[:, 1] - bounds[:, 0], np.exp(m.theta[1:])
    Xu = (X - lo) / span
    c = Xu.mean(0)
    Y = np.concatenate([(Xu - c) / ls, np.zeros((1, X.shape[1]))])
    Cn = ((Xc - lo) / span - c) / ls
    u = SCALE[kid] * ((Y[:, None, :] - Cn[None, :, :]) ** 2).sum(2)
    return u, SCALE[kid] * (Y * Y).sum(1), SCALE[kid] * (Cn * Cn).sum(1)


def _beside(rng, m, bounds, X, kid, ubnd, uhi, n, u_of=None, rows=None):
    """n candidates one step along one axis from a training row, u = u_of (default: 4 .. 40 ubnd) to that row and every other
    row (the padding row included) between 3 ubnd and uhi / 2: blocks of such candidates are skipped.  Returns them with
    their rows and axes."""
    lo, span, ls = bounds[:, 0], bounds[:, 1] - bounds[:, 0], np.exp(m.theta[1:])
    out, js, ks, sg = [], [], [], []
    for t in range(400 * n):
        if len(out) == n:
            break
        j = int(rng.integers(len(X))) if rows is None else int(rng.choice(rows[len(out) % len(rows)]))
        k, sign = int(rng.integers(X.shape[1])), float(rng.choice([-1.0, 1.0]))
        ut = ubnd * rng.uniform(4.0, 40.0) if u_of is None else u_of
        x = X[j].copy()
        x[k] += sign * ls[k] * span[k] * np.sqrt(ut / SCALE[kid])
        u = _u_all(m, bounds, X, kid, x[None, :])[0][:, 0]
        u[j] = 10.0 * ubnd      # (the designed pair itself)
        if u.min() >= 3.0 * ubnd and u.max() <= 0.5 * uhi:
            out.append(x); js.append(j); ks.append(k); sg.append(sign)
    assert len(out) == n, "no room beside the training rows for the designed candidates"
    return np.array(out), js, ks, sg


def _pool(rng, m, bounds, X, kid, M):
    """The pool, and the same pool with the rows of (c) and (e) replaced by ordinary far candidates, with what the two must
    differ by.  Candidates 0 .. 63 and 64 .. 127 are one wave each, halves of 32 are the blocks' columns.
    Wave 0, first half: (d) a NaN, an inf, a coordinate beyond FP32 (the wave never screens), (b) on and next to training rows.
    Wave 1: (e), u = ubnd + s delta to one training row with delta the one this wave has for that row's workgroup; s > 0 in the
    first half (with far candidates: those blocks are skipped, by the FP64 test where s < 1), s < 0 in the second (live).
    (c) beyond uhi: 4 rows among far candidates, in the second half of wave 2 (of wave 0 where the pool has no whole wave 2);
    the first half of wave 2 holds far candidates only.
    Behind them (a) uniform in the box, with more of (b)."""
    d, N = len(bounds), len(X)
    lo, span, ls = bounds[:, 0], bounds[:, 1] - bounds[:, 0], np.exp(m.theta[1:])
    sc, uhi = SCALE[kid], 1e6 if kid == 0 else 1e12
    ubnd = _ubnd(kid, float(np.exp(m.theta[0])), float(np.abs(m.alpha_).sum()))
    Xc = rng.uniform(bounds[:, 0], bounds[:, 1], (M, d))
    Xc[0, rng.integers(d)] = np.nan
    Xc[1, rng.integers(d)] = np.inf
    Xc[2, int(np.argmin(ls))] = 1e36
    idx = rng.integers(0, N, 8)
    Xc[3:11] = X[idx] + rng.normal(0, 1, (8, d)) * ls * span * rng.choice([0.0, 0.5, 3.0], (8, 1))
    if M > 400:
        n_b = M // 20
        idx = rng.integers(0, N, n_b)
        Xc[192:192 + n_b] = X[idx] + rng.normal(0, 1, (n_b, d)) * ls * span * rng.choice([0.0, 0.5, 3.0], (n_b, 1))
    Xc[64:128] = _beside(rng, m, bounds, X, kid, ubnd, uhi, 64)[0]
    c0 = 160 if M >= 192 else 32
    Xc[c0:c0 + 32] = _beside(rng, m, bounds, X, kid, ubnd, uhi, 32)[0]
    if c0 == 160:       # (the other half of that wave: far candidates as well, so that its blocks are known to be skipped)
        Xc[128:160] = _beside(rng, m, bounds, X, kid, ubnd, uhi, 32)[0]
    Xb = Xc.copy()
    # (c): along the axis of the shortest length scale, at least 1.5 sqrt(uhi / SC) scaled units beyond the box: u >= 2.25 uhi
    kmin = int(np.argmin(ls))
    Xc[c0:c0 + 4, kmin] = bounds[kmin, 1] + span[kmin] * ls[kmin] * np.sqrt(uhi / sc) * rng.uniform(1.5, 2.0, 4)
    assert _u_all(m, bounds, X, kid, Xc[c0:c0 + 4])[0].min() > 2.0 * uhi
    # (e): the rows, axes and directions first (u = ubnd), then delta of the wave as it then stands, then the steps
    nrb = -(-N // 16)
    rows = [np.arange(16 * b, min(16 * b + 16, N)) for b in rng.permutation(nrb)]
    s_all = S_NEAR + S_FAR + S_BELOW
    xe, je, ke, se = _beside(rng, m, bounds, X, kid, ubnd, uhi, len(s_all), u_of=ubnd, rows=rows)
    n_pos = len(S_NEAR) + len(S_FAR)
    slots = list(range(64, 64 + n_pos)) + list(range(96, 96 + len(S_BELOW)))
    Xc[slots] = xe
    _, yn, xn = _u_all(m, bounds, X, kid, Xc[64:128])
    for t, (s, j, k, sign) in enumerate(zip(s_all, je, ke, se)):
        ymax = yn[128 * (j // 128):min(128 * (j // 128) + 128, N)].max()
        delta = 2.0 ** -24 * (d + 8) * (np.sqrt(ymax) + np.sqrt(xn.max())) ** 2
        Xc[slots[t]] = X[j]
        Xc[slots[t], k] += sign * ls[k] * span[k] * np.sqrt(max(ubnd + s * delta, 0.0) / sc)
    u = _u_all(m, bounds, X, kid, Xc[64:96])[0]
    assert u.min() >= ubnd and u.max() <= 0.5 * uhi         # the first half of wave 1: every block is skipped
    # Wave 2 with (c) in it: the norms of (c) enter the wave's delta (at uhi = 1e12 it exceeds ubnd many times over), and the
    # blocks of the wave's other half, far candidates all, are certified only where every u clears ubnd + delta.
    sure, maybe = 0, 0
    if c0 == 160:
        u2, _, xn2 = _u_all(m, bounds, X, kid, Xc[128:192])
        for b in range(-(-N // 128) * 8):
            r = [min(q, N) for q in range(16 * b, 16 * b + 16)]        # (row N of u2: the zero padding row)
            real = yn[128 * (b // 8):min(128 * (b // 8) + 128, N)]
            delta = 2.0 ** -24 * (d + 8) * (np.sqrt(real.max()) + np.sqrt(xn2.max())) ** 2
            blk = u2[r][:, :32]
            # (u32 is within the margin of these pairs' own norms of u, whatever the wave's delta is)
            own = 2.0 ** -24 * (d + 8) * (np.sqrt(real.max()) + np.sqrt(xn2[:32].max())) ** 2
            if blk.min() + own < ubnd + delta:
                sure += 1
            elif not (blk.min() - own >= ubnd + delta and blk.max() + own <= uhi - delta):
                maybe += 1
    expect = dict(live=-(-N // 128) * 8 + len({j // 16 for j in je[n_pos:]}),         # (c): every row block; s < 0: theirs
                  fall_min=len({j // 16 for j in je[:len(S_NEAR)]}), fall_max=len({j // 16 for j in je[:n_pos]}),
                  # (where (c) shares wave 0, which never screens, the far candidates in its place are left to the FP64 test;
                  # in wave 2 the blocks of the other half are, where (c) has raised delta above them)
                  fall_c=-(-N // 128) * 8 if c0 == 32 else -sure, fall_maybe=maybe)
    return Xc, Xb, expect


def _stage_a(dev, sweep, screen, **opts):
    """Stage A of a pruned sweep as it stands (test hook "panel_debug" & 256), its statistics, then the completion."""
    dev.set_option("sweep_screen", screen)
    for k, v in opts.items():
        dev.set_option(k, v)
    dev.set_option("sweep_prune", 1)
    try:
        sweep(True)
    finally:
        dev.set_option("sweep_prune", 0)
    info, scr = dev.sweep_prune_info(), dev.sweep_screen_info()
    dev.set_option("panel_debug", 256)
    try:
        st = dev.sweep_fetch(("y", "acq"))
    finally:
        dev.set_option("panel_debug", 0)
    top = dev.sweep_topk(16)
    info.update({k: v for k, v in dev.sweep_prune_info().items() if k in ("survivors", "rounds", "contracted")})
    done = dev.sweep_fetch(("y", "sigma", "acq"))
    return info, scr, st, done, top


def _reset(dev):
    for k, v in (("sweep_prune", 0), ("sweep_chunk", 0), ("sweep_mean_bound", 1), ("sweep_screen", 1), ("panel_debug", 0)):
        dev.set_option(k, v)


@functools.lru_cache(maxsize=None)
def _device():
    from gpry_amd import _lib
    return _lib.Device(0)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Runs case i once and returns what the coverage test counts."""
    import fuzz_prune as fz
    from gpry_amd import _lib
    from oracle import gpry_oracle as orc
    from test_sweep_mean_bound_gpu import _short_model
    N, d, M, chunk, kid, with_mask = CASES[i]
    rng = np.random.default_rng(500 + i)
    dev = _device()
    m, bounds, X = _short_model(rng, orc, d, kid, N)
    if d <= 3:      # (one ordinary length scale out of one or three keeps the matrix-pipe form: all of them at 1e-3 of the box)
        m.theta[1:] = np.log(1e-3)
        m.newly_appended = 1
        m._update_model()
    Xc, Xb, expect = _pool(rng, m, bounds, X, kid, M)
    mask = None
    if with_mask:
        mask = (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_CLASSIFIED_INF
        mask |= (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_OUTSIDE_TRUST
    zeta, base, sn = orc.auto_zeta(d), m.y_max, m.noise_level
    try:
        dev.set_train(m.X_train_, m.y_train_, m.alpha)
        dev.set_theta(kid, m.theta)
        dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
        assert dev.factorize() == 0
        dev.set_option("sweep_chunk", chunk)

        def sweep(prune, **kw):
            return dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, M=M, want=() if prune else ("y", "sigma", "acq"), **kw)

        full = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask)
        on = _stage_a(dev, sweep, 1)
        off = _stage_a(dev, sweep, 0)
        hybrid = dev.sweep_info()["panel_form"] == "hybrid"
        for k in ("y", "acq"):      # stage A, NaN positions included
            assert np.array_equal(on[2][k], off[2][k], equal_nan=True) and np.array_equal(np.isnan(on[2][k]), np.isnan(off[2][k])), k
        for k in INFO_KEYS:
            assert on[0][k] == off[0][k], (k, on[0], off[0])
        for k in ("y", "sigma", "acq"):     # the completion: the full sweep's bit for bit
            assert np.array_equal(on[3][k], full[k], equal_nan=True), k
            assert np.array_equal(off[3][k], full[k], equal_nan=True), k
        for f in fz.FIELDS:     # (the shortlist of a pool with NaN rows may hold them)
            assert np.array_equal(on[4][0][f], off[4][0][f], equal_nan=True), (f, on[4][0][f], off[4][0][f])
        assert on[4][1] == off[4][1]
        info, scr = on[0], on[1]
        cert, blocks, live = scr["certified"], info["blocks"], info["live_blocks"]
        print(f"case {i} N={N} d={d} M={M} chunk={chunk} kid={kid} mask={with_mask}: form "
              f"{dev.sweep_info()['panel_form']}, y_bound {info['y_bound']}, blocks {blocks}, live {live}, certified {cert}")
        assert hybrid and info["y_bound"] == 1      # (every case is built to take the hybrid form and the bound pass)
        assert scr["blocks"] == blocks and 0 <= cert <= blocks - live
        assert off[1]["certified"] == 0
        # The same pool with (c) and (e) replaced by far candidates.  (c): its blocks are live, so never certified.  (e), s < 0:
        # live.  (e), 0 < s < 1: the screen leaves the block to the FP64 test, which skips it -- a kernel without the margin,
        # or with its sign wrong, certifies these and the count of such blocks does not move.
        def sweep_b(prune, **kw):
            return dev.sweep_logexp(Xb, zeta, base, sn, mask=mask, M=M, want=(), **kw)

        bi, bs = _stage_a(dev, sweep_b, 1)[:2]
        fall, fall_b = blocks - live - cert, bi["blocks"] - bi["live_blocks"] - bs["certified"]
        print(f"  without (c) and (e): live {bi['live_blocks']}, certified {bs['certified']}; left to the FP64 test and skipped: "
              f"{fall} with, {fall_b} without; expected {expect}")
        assert bi["blocks"] == blocks and live - bi["live_blocks"] == expect["live"], (live, bi["live_blocks"], expect)
        assert expect["fall_min"] >= 1 and expect["fall_min"] <= fall - fall_b + expect["fall_c"] <= expect["fall_max"] + expect["fall_maybe"], (fall, fall_b, expect)
        # The shortlists of the pruned sweep against the full sweep's (default options: the screen is on).  The harness
        # compares arrays with == and cannot take a pool with NaNs: it gets the same pool with the three rows of (d) redrawn.
        Xf = Xc.copy()
        Xf[:3] = rng.uniform(bounds[:, 0], bounds[:, 1], (3, d))

        def sweep_f(prune, **kw):
            return dev.sweep_logexp(Xf, zeta, base, sn, mask=mask, M=M, want=() if prune else ("y", "sigma", "acq"), **kw)

        full_f = dev.sweep_logexp(Xf, zeta, base, sn, mask=mask)
        a = full_f["acq"]
        fin = np.isfinite(a)
        series = fz._series(rng, M, np.where(fin, a, -np.inf), int(fin.sum()), None)
        dev.set_option("sweep_screen", 1)
        bad, _ = fz._pruned_against_full(i, dev, Counter(), sweep_f, M, series, full_f, "screen=1")
        assert bad == 0
        # no bound pass, no certified blocks: the option "sweep_mean_bound" off, and the sampler's y
        nb = _stage_a(dev, sweep, 1, sweep_mean_bound=0)
        assert nb[0]["y_bound"] == 0 and nb[1]["certified"] == 0
        dev.set_option("sweep_mean_bound", 1)
        dev.set_option("sweep_prune", 1)
        try:
            dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, M=M, want=(), y_given=np.nan_to_num(full["y"]))
        finally:
            dev.set_option("sweep_prune", 0)
        assert dev.sweep_prune_info()["y_bound"] == 0 and dev.sweep_screen_info()["certified"] == 0
    finally:
        _reset(dev)
    return dict(hybrid=hybrid and bool(info["y_bound"]), cert=cert, blocks=blocks, live=live, M=M)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_screen_on_and_off_give_the_same_sweep(i):
    res = _case(i)
    if res["M"] == 5000:
        # far candidates dominate these pools: the screen certifies what the emulation says it does (test_sweep_screen_cpu.py)
        assert res["blocks"] - res["live"] >= 100 and res["cert"] >= 0.95 * (res["blocks"] - res["live"]), res


def test_screen_was_exercised():
    res = [_case(i) for i in range(len(CASES))]
    partly = sum(1 for r in res if 0 < r["cert"] < r["blocks"])
    print(f"cases with 0 < certified < blocks: {partly}; without a bound pass: {sum(1 for r in res if not r['hybrid'])}")
    assert partly >= 5, res


def test_no_screen_without_the_hybrid_form():
    """Ordinary length scales: the model takes another panel form, stage A computes y, nothing is certified."""
    from oracle import gpry_oracle as orc
    from test_sweep_mean_bound_gpu import _short_model
    rng = np.random.default_rng(77)
    dev = _device()
    m, bounds, X = _short_model(rng, orc, 3, 3, 129)
    m.theta[1:] = np.log(0.3)
    m.newly_appended = 1
    m._update_model()
    Xc = rng.uniform(bounds[:, 0], bounds[:, 1], (600, 3))
    try:
        dev.set_train(m.X_train_, m.y_train_, m.alpha)
        dev.set_theta(3, m.theta)
        dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
        assert dev.factorize() == 0
        full = dev.sweep_logexp(Xc, orc.auto_zeta(3), m.y_max, m.noise_level)
        info, scr, _, done, _ = _stage_a(dev, lambda prune: dev.sweep_logexp(Xc, orc.auto_zeta(3), m.y_max, m.noise_level, want=()), 1)
        assert dev.sweep_info()["panel_form"] != "hybrid"
        assert info["y_bound"] == 0 and scr == {"certified": 0, "blocks": 0}
        assert np.array_equal(done["acq"], full["acq"])
    finally:
        _reset(dev)


def test_screen_on_a_group_of_three_contexts():
    """Members inherit the default (on); the sharded pruned sweep ends in the arrays of the unpruned one with the screen on
    and off, and the members' certified counts are positive only with it on."""
    from gpry_amd import _lib
    from oracle import gpry_oracle as orc
    from test_sweep_mean_bound_gpu import _short_model
    N, d, M, kid = 129, 16, 5000, 3
    rng = np.random.default_rng(600)
    dev = _device()
    m, bounds, X = _short_model(rng, orc, d, kid, N)
    Xc = _pool(rng, m, bounds, X, kid, M)[0]
    zeta, base, sn = orc.auto_zeta(d), m.y_max, m.noise_level
    grp = _lib.DeviceGroup([0, 0, 0], adopt=dev)
    try:
        dev.set_train(m.X_train_, m.y_train_, m.alpha)
        dev.set_theta(kid, m.theta)
        dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
        assert dev.factorize() == 0
        grp.set_model(m.X_train_, m.y_train_, m.alpha, kid, m.theta,
                      (m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi()))
        members = [grp.member(j) for j in range(grp.size)]
        grp.sweep_logexp(Xc, zeta, base, sn, want=("acq",))
        full = grp.sweep_fetch(("y", "sigma", "acq"))
        ftop = grp.sweep_topk(64)
        stats = {}
        for screen in (None, 0):        # None: what the members were created with
            for mb in members:
                if screen is not None:
                    mb.set_option("sweep_screen", screen)
                mb.set_option("sweep_prune", 1)
            try:
                grp.sweep_logexp(Xc, zeta, base, sn, want=())
            finally:
                for mb in members:
                    mb.set_option("sweep_prune", 0)
            stats[screen] = [(mb.sweep_prune_info(), mb.sweep_screen_info()) for mb in members]
            top = grp.sweep_topk(64)
            n = len(top[0])     # (a member's pruned bound may hold back more: a prefix of the unpruned list)
            assert n <= len(ftop[0]) and all(np.array_equal(top[0][f], ftop[0][f][:n]) for f in ("idx", "acq", "y", "sigma"))
            got = grp.sweep_fetch(("y", "sigma", "acq"))
            for k in ("y", "sigma", "acq"):
                assert np.array_equal(got[k], full[k], equal_nan=True), (screen, k)
        for (i_on, s_on), (i_off, s_off) in zip(stats[None], stats[0]):
            assert i_on["y_bound"] == i_off["y_bound"] and i_on["live_blocks"] == i_off["live_blocks"] and i_on["blocks"] == i_off["blocks"]
            assert 0 <= s_on["certified"] <= i_on["blocks"] - i_on["live_blocks"] and s_off["certified"] == 0
        print("group members (live, blocks, certified):", [(a["live_blocks"], a["blocks"], b["certified"]) for a, b in stats[None]])
        assert all(a["y_bound"] == 1 for a, _ in stats[None])
        assert all(b["certified"] > 0 for _, b in stats[None])
    finally:
        grp.close()
        _reset(dev)
