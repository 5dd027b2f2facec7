#!/usr/bin/env python3
"""Randomised exactness sweep of the pruned NORA sweep (option "sweep_prune") and of the sweep with sampler-supplied y
(gpry_sweep_logexp_given): random N around the padding quanta, d in 1..32, all four kernels, every panel form, pools from
one row to a few 1e5 (resident or uploaded chunk by chunk underneath the sweep), caller masks, device gates, exclusions,
duplicate rows, rows on training points and a block of far rows whose acquisitions tie bit for bit.

Per case the pruned shortlists (a series of growing K with changing exclusions on one sweep) are the full sweep's records
bit for bit, the pruned bound is >= the full one and the fetched arrays are the full sweep's; the sigma-only sweep gives
the ordinary sweep's sigma; both-given is LogExp.f; and the full sweep agrees with the oracle on a random subset and on
every row that can reach the shortlist.  ``run`` returns (violations, worst deviations, coverage tally)."""
import os
import sys
import time
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gpry_amd import _lib  # noqa: E402
from oracle import gpry_oracle as orc  # noqa: E402

FIELDS = ("idx", "acq", "y", "sigma")
N_CHOICES = (1, 2, 17, 127, 128, 129, 255, 257, 1000, 2048, 2049, 4096)
M_CHOICES = (1, 127, 128, 129, 1000, 5000, 20000, 100000, 300000)
TOL_MEAN, TOL_VAR, TOL_ACQ = 1e-7, 1e-8, 1e-4      # tests/tools/fuzz_parity.py
ORACLE_BLOCK = 2048                                 # rows of K* the oracle builds at a time


def run(n_cases=20, seed=0, dev=None, group=True):
    """Returns (number of violations, worst deviations, coverage tally)."""
    rng = np.random.default_rng(seed)
    dev = dev or _lib.Device(0)
    worst = {"mean": 0.0, "var": 0.0, "acq": 0.0}
    cov = Counter()
    bad = 0
    for case in range(n_cases):
        try:
            bad += _one_case(case, rng, dev, worst, cov, group)
        finally:
            for k, v in (("sweep_prune", 0), ("sweep_chunk", 0), ("cross_mfma", 1), ("cross_hybrid", 1)):
                dev.set_option(k, v)
            dev.set_gates()
    return bad, worst, cov


def oracle_predict(m, X):
    """OracleGPR.predict(return_std=True) in blocks of rows (K* of 1e5 x 4096 is 3 GB in one piece)."""
    mu, sd = np.empty(len(X)), np.empty(len(X))
    for i in range(0, len(X), ORACLE_BLOCK):
        a, b = m.predict(X[i:i + ORACLE_BLOCK], return_std=True)
        mu[i:i + ORACLE_BLOCK], sd[i:i + ORACLE_BLOCK] = a, b
    return mu, sd


def _draw_model(rng):
    N = int(rng.choice(N_CHOICES))
    d = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 21, 27, 32])) if rng.random() < 0.5 else int(rng.integers(1, 33))
    kid = int(rng.integers(0, 4))
    bounds = np.stack([-rng.uniform(1, 6, d), rng.uniform(1, 6, d)], axis=1)
    X = rng.uniform(bounds[:, 0], bounds[:, 1], (N, d))
    y = -0.5 * ((X / (bounds[:, 1] - bounds[:, 0])) ** 2).sum(1) * rng.uniform(1, 30) + rng.normal(0, 0.01, N)
    m = orc.OracleGPR(bounds, kernel_id=kid, normalize_y=(N > 1), noise_level=float(10 ** rng.uniform(-3, -1)),
                      clip_factor=float(rng.choice([1.0, 1.1, 2.0])))
    r = rng.random()
    if r < 0.2:             # length scales far below the extent of the data: the gate fails through R^2 (hybrid form)
        ls = 10 ** rng.uniform(-3, -2, d)
    elif r < 0.3:           # long length scales: a nearly singular K (the gate fails through the weights)
        ls = 10 ** rng.uniform(0.3, 1, d)
    else:
        ls = 10 ** rng.uniform(-0.7, 0.3, d)
    m.theta = np.log(np.concatenate(([10 ** rng.uniform(-1, 2)], ls)))
    m.fitted = True
    m.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    return m, bounds, X, kid


def _draw_pool(rng, m, bounds, X, M):
    d = len(bounds)
    N = len(X)
    Xc = rng.uniform(bounds[:, 0] - 0.2, bounds[:, 1] + 0.2, (M, d))
    n_far = 0
    if M >= 100 and rng.random() < 0.5:
        # far rows: k* = 0 for every panel form (the kernels underflow), so y = y_mean, sigma = the prior's and the
        # acquisition equals its bound bit for bit; they all tie
        n_far = int(min(M // 2, rng.choice([50, 500, 3000])))
        span = bounds[:, 1] - bounds[:, 0]
        far = bounds[:, 1] + span * (2000.0 * np.exp(m.theta[1:]).max() + 1.0)
        Xc[M - n_far:] = far + span * rng.uniform(0, 1, (n_far, d))
    if M > 8:
        k = max(1, min(M // 8, 64))
        dst = rng.choice(M - n_far, size=min(k, M - n_far), replace=False)
        Xc[dst] = X[rng.integers(0, N, len(dst))]                       # candidates on training points
        src = rng.integers(0, M, k)
        dst = rng.integers(0, M - n_far, k)
        Xc[dst] = Xc[src]                                               # duplicate rows (far ones too, outside the block)
    return Xc, n_far


def _gates(rng, m, bounds, cov):
    """Random SVM (support vectors in the unit cube of the affine map) and / or trust box; the host's verdict and a flag
    for rows whose decision value is too close to 0 to be called either way."""
    d = len(bounds)
    kw = {}
    if rng.random() < 0.6:
        n_sv = int(rng.integers(1, 40))
        kw.update(sv=rng.uniform(0, 1, (n_sv, d)), coef=rng.normal(0, 1, n_sv), gamma=float(rng.uniform(0.5, 4.0)),
                  intercept=float(rng.normal(0, 0.3)), positive_is_finite=bool(rng.random() < 0.7))
    if not kw or rng.random() < 0.5:
        lo = bounds[:, 0] + rng.uniform(0, 0.3, d) * (bounds[:, 1] - bounds[:, 0])
        hi = bounds[:, 1] - rng.uniform(0, 0.3, d) * (bounds[:, 1] - bounds[:, 0])
        kw["trust_bounds"] = np.stack([lo, hi], axis=1)
    cov["gates_svm" if "sv" in kw else "gates_trust"] += 1

    def verdict(Xc):
        bits = np.zeros(len(Xc), np.uint8)
        unsure = np.zeros(len(Xc), bool)
        if "trust_bounds" in kw:
            tb = kw["trust_bounds"]
            bits[~np.all((Xc >= tb[:, 0]) & (Xc <= tb[:, 1]), axis=1)] |= _lib.MASK_OUTSIDE_TRUST
        if "sv" in kw:
            Xu = m.pre_X.transform(Xc)
            dec = np.full(len(Xc), kw["intercept"])
            for s, c in zip(kw["sv"], kw["coef"]):
                dec += c * np.exp(-kw["gamma"] * ((Xu - s) ** 2).sum(1))
            bits[(dec > 0) != kw["positive_is_finite"]] |= _lib.MASK_CLASSIFIED_INF
            unsure = np.abs(dec) < 1e-9 * (1.0 + np.abs(kw["coef"]).sum())
        return bits, unsure
    return kw, verdict


def _series(rng, M, acq_full, n_fin, tie_K):
    """(K, exclusions) of the repeated sweep_topk calls on one sweep: growing K, a new exclusion list each time."""
    Ks = [int(rng.choice([1, 16, 256]))]
    Ks.append(Ks[0] * int(rng.choice([2, 4, 16])))
    if tie_K is not None:
        Ks.append(tie_K)
    if rng.random() < 0.5 or n_fin < 2000:
        Ks.append(n_fin + int(rng.integers(0, 3)))          # K at or above the finite count
    Ks = sorted(set(max(1, k) for k in Ks))
    order = np.argsort(acq_full)[::-1]
    out = []
    for K in Ks:
        ex = None
        if rng.random() < 0.5 and M > 4:
            n_ex = int(rng.integers(1, min(M // 2, 40) + 1))
            ex = np.unique(np.concatenate([order[:2 * K][rng.integers(0, min(M, 2 * K), n_ex)],
                                           rng.integers(0, M, n_ex // 2 + 1)]))
        out.append((K, ex))
    return out


def _logexp_and_tol(y, sigma, base, sn, zeta):
    """LogExp.f and what one rounding more or less (the device's log against numpy's) can move it: a few ulps of its two
    terms, which may cancel."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = 2 * zeta * (y - base)
        lg = np.log(np.sqrt(np.clip(sigma ** 2 - sn ** 2, 0.0, None)))
        tol = 8 * np.finfo(float).eps * (np.abs(lin) + np.abs(lg) + 1e-300)
    return orc.logexp_f(y, sigma, base, sn, zeta), tol


def _records_equal(case, what, got, ref):
    for f in FIELDS:
        if not np.array_equal(got[f], ref[f]):
            n = min(len(got), len(ref))
            first = np.flatnonzero(got[f][:n] != ref[f][:n])
            print(f"case {case}: {what}: records differ in {f} (lengths {len(got)} / {len(ref)}, first at "
                  f"{first[:3] if first.size else n})")
            return False
    return True


def _pruned_against_full(case, dev, cov, sweep, M, series, full, tag):
    """Full sweep's shortlists, then the same on a pruned sweep: records, bounds, n_nan, fetch, prune outcomes.  Returns
    (violations, the panel form stage A recorded)."""
    bad = 0
    out = sweep(False)
    ref = [dev.sweep_topk(K, exclude=ex) for K, ex in series]
    arrays = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        if not np.array_equal(arrays[k], full[k]):
            print(f"case {case}: {tag}: a repeated full sweep differs in {k}"); bad += 1
    dev.set_option("sweep_prune", 1)
    try:
        pout = sweep(True)
    finally:
        dev.set_option("sweep_prune", 0)
    if pout["n_nan"] != out["n_nan"]:
        print(f"case {case}: {tag}: n_nan {pout['n_nan']} pruned, {out['n_nan']} full"); bad += 1
    if dev.sweep_prune_info()["pruned"] != 1:
        print(f"case {case}: {tag}: the sweep was not pruned"); bad += 1
    form = dev.sweep_info()["panel_form"]
    for (K, ex), (ft, fb) in zip(series, ref):
        pt, pb = dev.sweep_topk(K, exclude=ex)
        info = dev.sweep_prune_info()
        if info["completed"]:
            cov["outcome_completed"] += 1
        elif info["rounds"] == 1:
            cov["outcome_round1"] += 1
        elif info["survivors"] >= 0:
            cov["outcome_survivors"] += 1
        if not _records_equal(case, f"{tag} K={K}", pt, ft):
            bad += 1
        if not (pb >= fb):
            print(f"case {case}: {tag} K={K}: pruned bound {pb!r} < full bound {fb!r} ({info})"); bad += 1
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        if not np.array_equal(got[k], full[k]):
            print(f"case {case}: {tag}: the fetched {k} is not the full sweep's"); bad += 1
    if dev.sweep_prune_info()["pruned"] != 0:
        print(f"case {case}: {tag}: still pruned after the fetch"); bad += 1
    K, ex = series[-1]
    pt, pb = dev.sweep_topk(K, exclude=ex)          # completed: the full sweep's arrays, its bound
    if not _records_equal(case, f"{tag} after the fetch", pt, ref[-1][0]) or pb != ref[-1][1]:
        bad += 1
    return bad, form


def _one_case(case, rng, dev, worst, cov, group):
    bad = 0
    m, bounds, X, kid = _draw_model(rng)
    N, d = X.shape
    M = int(rng.choice(M_CHOICES))
    if N * M > 4096 * 100000 and rng.random() < 0.5:
        M = int(rng.choice([1000, 20000]))
    Xc, n_far = _draw_pool(rng, m, bounds, X, M)
    dev.set_train(m.X_train_, m.y_train_, m.alpha)
    dev.set_theta(kid, m.theta)
    dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
    if dev.factorize() != 0:
        print(f"case {case}: device says not PD (N={N} d={d} kid={kid})")
        return 1
    cov[f"kid{kid}"] += 1
    cov["N_le_128"] += N <= 128
    cov["d_1"] += d == 1
    cov["d_gt_20"] += d > 20
    r = rng.random()
    if r < 0.15:
        dev.set_option("cross_mfma", 0)                 # the difference form whatever the estimates say
    elif r < 0.3:
        dev.set_option("cross_hybrid", 0)               # a model that fails the gate: the difference form, not the hybrid
    chunk = int(rng.choice([1024, 32768]))
    dev.set_option("sweep_chunk", chunk)
    upload = bool(rng.random() < 0.5)
    mask = None
    if rng.random() < 0.4:
        mask = (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_CLASSIFIED_INF
        mask |= (rng.random(M) < 0.15).astype(np.uint8) * _lib.MASK_OUTSIDE_TRUST
    gates, verdict = None, None
    if rng.random() < 0.35:
        gates, verdict = _gates(rng, m, bounds, cov)
        dev.set_gates(**gates)
        if mask is None:
            cov["gates_no_mask"] += 1
    zeta = orc.auto_zeta(d) if rng.random() < 0.7 else float(10 ** rng.uniform(-2.5, 0.5))
    base, sn = m.y_max, m.noise_level
    cfg = f"N={N} d={d} M={M} kid={kid} chunk={chunk} upload={upload} mask={mask is not None} gates={gates is not None}"

    def sweep(prune, **kw):
        want = () if prune else ("y", "sigma", "acq")
        return dev.sweep_logexp(Xc if upload else None, zeta, base, sn, mask=mask, M=M, want=want, **kw)

    full = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask)         # (puts the pool on the device for the resident runs)
    a = full["acq"]
    if full["n_nan"] or np.isnan(a).any():
        print(f"case {case}: NaN in the full sweep ({cfg})")
        return bad + 1
    fin = np.isfinite(a)
    n_fin = int(fin.sum())
    # the tie block: far rows all at one value; K chosen so that the K-th place falls inside it
    tie_K = None
    if n_far:
        af = a[M - n_far:]
        af = af[np.isfinite(af)]
        if len(af) >= 2 and np.all(af == af[0]):
            above = int((a > af[0]).sum())
            n_eq = int((a == af[0]).sum())
            tie_K = above + max(1, n_eq // 2)
            cov["tie_at_K"] += 1
        elif len(af) and not np.all(af == af[0]):
            print(f"case {case}: the far rows do not tie ({cfg})"); bad += 1
    series = _series(rng, M, np.where(fin, a, -np.inf), n_fin, tie_K)
    cov["K_ge_finite"] += any(K >= n_fin for K, _ in series)
    cov["multichunk_upload"] += upload and M > chunk
    cov["multichunk_upload_gates"] += upload and M > chunk and gates is not None

    # --- the full sweep's shortlist order is the lexsort of its own acquisition
    K0 = series[0][0]
    top, _ = dev.sweep_topk(K0)
    order = np.lexsort((-np.arange(M), -a))
    if not np.array_equal(top["idx"], order[:len(top)]) or len(top) != min(K0, M):
        print(f"case {case}: the shortlist is not the lexsort of the full acquisition ({cfg})"); bad += 1

    # --- the ordinary sweep, pruned against full
    b, form = _pruned_against_full(case, dev, cov, sweep, M, series, full, "ordinary")
    bad += b
    cov[f"form_{form}"] += 1

    # --- against the oracle: a random subset, every shortlist row, every row that can reach the top K0
    t_K = a[order[min(K0, M) - 1]]
    reach = np.flatnonzero(a >= t_K - 10 * TOL_ACQ) if np.isfinite(t_K) else np.empty(0, np.int64)
    if len(reach) > 4000:
        reach = order[:4000]
    rows = np.unique(np.concatenate([rng.choice(M, min(M, 300), replace=False), top["idx"][:512], reach]))
    rm, rs = oracle_predict(m, Xc[rows])
    bits = np.zeros(len(rows), np.uint8) if mask is None else mask[rows].copy()
    sure = np.ones(len(rows), bool)
    if verdict is not None:
        gb, unsure = verdict(Xc[rows])
        bits |= gb
        sure = ~unsure
    rm[bits != 0] = -np.inf
    rs[(bits & _lib.MASK_CLASSIFIED_INF) != 0] = 0.0
    gy, gs = full["y"][rows], full["sigma"][rows]
    if not np.array_equal(np.isneginf(gy[sure]), np.isneginf(rm[sure])):
        print(f"case {case}: -inf pattern differs from the oracle's ({cfg})"); bad += 1
    ok = sure & np.isfinite(rm) & np.isfinite(gy)
    scale = max(1.0, np.max(np.abs(m.y_train)))
    C = np.exp(m.theta[0]) * m.pre_y.std_ ** 2
    e = np.max(np.abs(gy[ok] - rm[ok])) / scale if ok.any() else 0.0
    worst["mean"] = max(worst["mean"], e)
    if e > TOL_MEAN:
        print(f"case {case}: mean err {e:.2e} ({cfg}, form {form})"); bad += 1
    e = np.max(np.abs(gs[sure] ** 2 - rs[sure] ** 2)) / C if sure.any() else 0.0
    worst["var"] = max(worst["var"], e)
    if e > TOL_VAR:
        print(f"case {case}: var err {e:.2e} ({cfg}, form {form})"); bad += 1
    racq = orc.logexp_f(rm, rs, base, sn, zeta)
    okm = sure & np.isfinite(racq) & (rs ** 2 - sn ** 2 > 1e-6 * C)
    if okm.any():
        e = np.max(np.abs(a[rows][okm] - racq[okm]))
        worst["acq"] = max(worst["acq"], e)
        if e > TOL_ACQ:
            print(f"case {case}: acq err {e:.2e} ({cfg})"); bad += 1
    if len(reach) and K0 <= 256 and sure.all():
        # every row whose oracle acquisition clears the oracle's K0-th value by more than the tolerance is shortlisted
        o = np.where(okm, racq, a[rows])
        oK = np.sort(o)[::-1][min(K0, len(o)) - 1]
        must = rows[okm & (o > oK + TOL_ACQ)]
        if not np.isin(must, top["idx"]).all():
            print(f"case {case}: {np.setdiff1d(must, top['idx']).size} rows the oracle ranks clearly in the top {K0} "
                  f"are not shortlisted ({cfg})"); bad += 1

    # --- sigma only: the caller's y, sigma bit for bit the ordinary sweep's, pruned against full
    fy = np.isfinite(full["y"])
    yg = full["y"] + 0.1 * (np.std(full["y"][fy]) if fy.any() else 1.0) * rng.standard_normal(M)
    yg[rng.random(M) < 0.05] = -np.inf
    yg[rng.choice(M, min(M, 50), replace=False)] = float(np.max(full["y"][fy])) if fy.any() else 0.0     # ties
    yg[rng.choice(M, min(M, 3), replace=False)] = m.y_max + 1e3 * max(1.0, m.pre_y.std_)
    yg[~np.isfinite(full["y"]) & (rng.random(M) < 0.5)] = m.y_max     # masked rows with a finite given y
    gfull = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, y_given=yg)
    if not np.array_equal(gfull["sigma"], full["sigma"]):
        print(f"case {case}: sigma of the sigma-only sweep differs from the ordinary sweep's ({cfg})"); bad += 1
    if not np.array_equal(gfull["y"], yg):
        print(f"case {case}: the sigma-only sweep changed the given y ({cfg})"); bad += 1
    ga, gt = _logexp_and_tol(yg, gfull["sigma"], base, sn, zeta)
    if not np.array_equal(np.isneginf(gfull["acq"]), np.isneginf(ga)):
        print(f"case {case}: sigma-only -inf pattern differs from LogExp.f ({cfg})"); bad += 1
    okg = np.isfinite(ga)
    if okg.any() and not (np.abs(gfull["acq"][okg] - ga[okg]) <= gt[okg]).all():
        print(f"case {case}: sigma-only acquisition is not LogExp.f of its y and sigma ({cfg})"); bad += 1
    gseries = _series(rng, M, gfull["acq"], int(np.isfinite(gfull["acq"]).sum()), None)

    def gsweep(prune):
        want = () if prune else ("y", "sigma", "acq")
        return dev.sweep_logexp(Xc if upload else None, zeta, base, sn, mask=mask, M=M, want=want, y_given=yg)
    bad += _pruned_against_full(case, dev, cov, gsweep, M, gseries, gfull, "sigma-only")[0]
    cov["sigma_only_pruned"] += 1

    # the sweep's own y handed back: the ordinary sweep's arrays and shortlists, full and pruned
    def osweep(prune):
        want = () if prune else ("y", "sigma", "acq")
        return dev.sweep_logexp(Xc if upload else None, zeta, base, sn, mask=mask, M=M, want=want, y_given=full["y"])
    same = osweep(False)
    if not (np.array_equal(same["acq"], full["acq"]) and np.array_equal(same["sigma"], full["sigma"])):
        print(f"case {case}: the sweep's own y handed back does not give its acquisition ({cfg})"); bad += 1
    else:
        bad += _pruned_against_full(case, dev, cov, osweep, M, series, full, "own y")[0]

    # --- both given: LogExp.f and nothing else
    sg = np.abs(full["sigma"]) * rng.uniform(0.5, 1.5, M)
    sg[rng.random(M) < 0.05] = 0.0
    both = dev.sweep_logexp(Xc, zeta, base, sn, mask=mask, y_given=yg, sigma_given=sg)
    ob, bt = _logexp_and_tol(yg, sg, base, sn, zeta)
    fo = np.isfinite(ob)
    if not (np.array_equal(np.isneginf(both["acq"]), np.isneginf(ob)) and (np.abs(both["acq"][fo] - ob[fo]) <= bt[fo]).all()):
        print(f"case {case}: both-given acquisition is not LogExp.f ({cfg})"); bad += 1

    # --- a 3-context group (member 0 the context above): pruned against unpruned
    if group and M >= 3 and rng.random() < 0.25:
        bad += _group_case(case, dev, m, kid, gates, Xc, mask, zeta, base, sn, series, cfg)
        cov["group"] += 1
    return bad


def _group_case(case, dev, m, kid, gates, Xc, mask, zeta, base, sn, series, cfg):
    bad = 0
    M = len(Xc)
    grp = _lib.DeviceGroup([0, 0, 0], adopt=dev)
    try:
        grp.set_model(m.X_train_, m.y_train_, m.alpha, kid, m.theta,
                      (m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi()))
        grp.set_gates(**(gates or {}))
        members = [grp.member(i) for i in range(grp.size)]
        res = {}
        for prune in (False, True):
            for mb in members:
                mb.set_option("sweep_prune", int(prune))
            try:
                out = grp.sweep_logexp(Xc, zeta, base, sn, mask=mask, want=() if prune else ("acq",))
            finally:
                for mb in members:
                    mb.set_option("sweep_prune", 0)
            res[prune] = [grp.sweep_topk(-(-2 * K // grp.size), exclude=ex) for K, ex in series]
            res[prune].append(grp.sweep_fetch(("y", "sigma", "acq")))
            if not prune and out["n_nan"]:
                print(f"case {case}: group: NaN ({cfg})"); bad += 1
        for (fr, fb, fe), (pr, pb, pe) in zip(res[False][:-1], res[True][:-1]):
            # a member's pruned bound is >= its full one, so the merge may hold back more: the pruned list is a prefix
            if not (len(pr) <= len(fr) and _records_equal(case, "group", pr, fr[:len(pr)]) and pb >= fb and pe == fe):
                print(f"case {case}: group: pruned shortlist is not the full one ({len(pr)} / {len(fr)} records, bounds "
                      f"{pb!r} / {fb!r}; {cfg})"); bad += 1
        for k in ("y", "sigma", "acq"):
            if not np.array_equal(res[True][-1][k], res[False][-1][k]):
                print(f"case {case}: group: fetched {k} differs ({cfg})"); bad += 1
    finally:
        grp.close()
    return bad


if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    t0 = time.time()
    bad, worst, cov = run(n_cases, seed)
    print(f"{n_cases} cases in {time.time() - t0:.1f} s; worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("coverage: " + ", ".join(f"{k} {v}" for k, v in sorted(cov.items())) + f"; violations: {bad}")
    sys.exit(1 if bad else 0)
