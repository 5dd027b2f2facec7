"""The bound pass of the pruned sweep (option "sweep_mean_bound"): stage A bounds y instead of computing it, and y is computed
exactly only for the candidates that are contracted.  On models in the short-length-scale regime that takes the hybrid panel
form, with the bound on and off: the shortlists are the full sweep's records bit for bit (tests/tools/fuzz_prune.py), the
stage-A bounds of y and of the acquisition are >= the full sweep's values elementwise, the fetched arrays are the full sweep's,
and the same holds on a 3-context group."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

D_CHOICES = (1, 2, 3, 5, 8, 13, 16, 21, 27, 32)
N_CHOICES = (17, 129, 257, 1000, 2049, 4096)


def _short_model(rng, orc, d, kid, N):
    bounds = np.stack([-rng.uniform(1, 6, d), rng.uniform(1, 6, d)], axis=1)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (N, d))
    y = -0.5 * ((X / (bounds[:, 1] - bounds[:, 0])) ** 2).sum(1) * rng.uniform(1, 30) + rng.normal(0, 0.01, N)
    m = orc.OracleGPR(bounds, kernel_id=kid, normalize_y=True, noise_level=float(10 ** rng.uniform(-3, -2.5)),
                      clip_factor=float(rng.choice([1.0, 1.1, 2.0])))
    ls = 10 ** rng.uniform(-3, -2.3, d)
    ls[: max(1, d // 3)] = 10 ** rng.uniform(-1.3, 0.3, max(1, d // 3))     # a few ordinary ones, as the bench's fit has
    m.theta = np.log(np.concatenate(([10 ** rng.uniform(-1, 2)], ls)))
    m.fitted = True
    m.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    return m, bounds, X


def _bound_checks(case, dev, sweep, full, cov):
    """Stage A with the bound pass: y and acq as they stand (test hook "panel_debug" & 256) are >= the full sweep's."""
    bad = 0
    dev.set_option("sweep_prune", 1)
    try:
        sweep(True)
    finally:
        dev.set_option("sweep_prune", 0)
    info = dev.sweep_prune_info()
    if dev.sweep_info()["panel_form"] != "hybrid":
        return bad, info
    if info["y_bound"] != 1 or not (0 <= info["live_blocks"] <= info["blocks"]) or info["blocks"] <= 0:
        print(f"case {case}: the bound pass did not run as it should ({info})")
        return bad + 1, info
    live, blocks = info["live_blocks"], info["blocks"]
    cov["bound_none_live" if live == 0 else "bound_all_live" if live == blocks else "bound_partly_live"] += 1
    dev.set_option("panel_debug", 256)
    try:
        st = dev.sweep_fetch(("y", "sigma", "acq"))
    finally:
        dev.set_option("panel_debug", 0)
    for k in ("y", "acq"):
        a, b = st[k], full[k]
        if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.all((a >= b) | np.isnan(b)):
            print(f"case {case}: the stage-A {k} is not an upper bound of the full sweep's "
                  f"({int(np.sum(a < b))} rows below)"); bad += 1
    pruned = st["sigma"] == -1.0
    if not np.array_equal(st["y"][~pruned], full["y"][~pruned]):      # (nothing contracted yet: all of them are bounds)
        print(f"case {case}: a contracted row's y is not exact"); bad += 1
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        if not np.array_equal(got[k], full[k]):
            print(f"case {case}: after the completion {k} is not the full sweep's"); bad += 1
    return bad, info


def _one_case(case, rng, dev, fz, orc, _lib, cov):
    bad = 0
    d = int(rng.choice(D_CHOICES))
    kid = int(rng.choice([0, 2, 3]))               # (Matern-1/2 never takes the matrix-pipe forms)
    N = int(rng.choice(N_CHOICES))
    m, bounds, X = _short_model(rng, orc, d, kid, N)
    M = int(rng.choice([129, 5000, 40000, 100000]))
    Xc, n_far = fz._draw_pool(rng, m, bounds, X, M)
    if rng.random() < 0.15:         # far rows only: beyond uhi every pair counts as live (tests the conservative side)
        span = bounds[:, 1] - bounds[:, 0]
        Xc = bounds[:, 1] + span * (2000.0 * np.exp(m.theta[1:]).max() + 1.0) + span * rng.uniform(0, 1, (M, d))
        n_far = M
    dev.set_train(m.X_train_, m.y_train_, m.alpha)
    dev.set_theta(kid, m.theta)
    dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
    if dev.factorize() != 0:
        print(f"case {case}: device says not PD (N={N} d={d} kid={kid})")
        return 1
    chunk = int(rng.choice([1024, 32768]))
    dev.set_option("sweep_chunk", chunk)
    upload = bool(rng.random() < 0.5)
    mask = None
    if rng.random() < 0.4:
        mask = (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_CLASSIFIED_INF
        mask |= (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_OUTSIDE_TRUST
    gates = None
    if rng.random() < 0.3:
        gates, _ = fz._gates(rng, m, bounds, cov)
        dev.set_gates(**gates)
    zeta = orc.auto_zeta(d) if rng.random() < 0.7 else float(10 ** rng.uniform(-2.5, 0.5))
    base, sn = m.y_max, m.noise_level

    def sweep(prune, **kw):
        want = () if prune else ("y", "sigma", "acq")
        return dev.sweep_logexp(Xc if upload else None, zeta, base, sn, mask=mask, M=M, want=want, **kw)

    full = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask)
    a = full["acq"]
    fin = np.isfinite(a)
    tie_K = None
    if n_far:
        af = a[M - n_far:]
        af = af[np.isfinite(af)]
        if len(af) >= 2 and np.all(af == af[0]):
            tie_K = int((a > af[0]).sum()) + max(1, int((a == af[0]).sum()) // 2)
            cov["tie_at_K"] += 1
    series = fz._series(rng, M, np.where(fin, a, -np.inf), int(fin.sum()), tie_K)
    for bound in (1, 0):
        dev.set_option("sweep_mean_bound", bound)
        b, form = fz._pruned_against_full(case, dev, cov, sweep, M, series, full, f"bound={bound}")
        bad += b
        info = dev.sweep_prune_info()
        cov[f"form_{form}"] += 1
        if bound == 0 and info["y_bound"] != 0:
            print(f"case {case}: the bound pass ran with the option off"); bad += 1
    dev.set_option("sweep_mean_bound", 1)
    b, info = _bound_checks(case, dev, sweep, full, cov)
    bad += b
    # the sampler-supplied y: no bound pass
    dev.set_option("sweep_prune", 1)
    try:
        dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, M=M, want=(), y_given=full["y"])
    finally:
        dev.set_option("sweep_prune", 0)
    if dev.sweep_prune_info()["y_bound"] != 0:
        print(f"case {case}: the bound pass ran on a sweep with y given"); bad += 1
    if rng.random() < 0.3 and M >= 3:
        bad += fz._group_case(case, dev, m, kid, gates, Xc, mask, zeta, base, sn, series, f"N={N} d={d} kid={kid}")
        cov["group"] += 1
    return bad


@pytest.mark.timeout(1200)
def test_bound_pass_keeps_records_and_arrays_of_the_full_sweep():
    import fuzz_prune as fz
    from gpry_amd import _lib
    from oracle import gpry_oracle as orc
    dev = _lib.Device(0)
    cov = Counter()
    bad = 0
    for seed in (31, 32):
        rng = np.random.default_rng(seed)
        for case in range(10):
            try:
                bad += _one_case(case, rng, dev, fz, orc, _lib, cov)
            finally:
                for k, v in (("sweep_prune", 0), ("sweep_chunk", 0), ("sweep_mean_bound", 1), ("panel_debug", 0)):
                    dev.set_option(k, v)
                dev.set_gates()
    print(f"coverage: {dict(sorted(cov.items()))}")
    assert bad == 0
    assert cov["form_hybrid"] >= 10 and cov["bound_partly_live"] >= 5 and cov["group"] >= 2, dict(cov)
