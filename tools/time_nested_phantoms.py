"""Phantom points of the nested sampler on the bench's fitted model (BASELINE configs[2]: N = 4096, d = 16) at the
reference's defaults (nlive 400, num_repeats 80, nprior 4000, 200 chains per generation), and their statistics on an
analytic Gaussian.

    python tools/time_nested_phantoms.py gen [--reps 7] [--plain-only] [--json out.json]
        device / wall time of the first generation of a run: gpry_ns_generation against gpry_ns_generation_phantoms at
        thin 1, 2 and 5, alternating, medians after a warm-up round.  --plain-only: only the existing entry point (for a
        checkout that has no other, such as the parent commit's).
    python tools/time_nested_phantoms.py runs [--runs 2] [--json out.json]
        full runs with phantoms off / thin 1 / 2 / 5: rows, ESS, device and wall time, host time of merged_weights;
        then NORA.multi_add with the grown pool: time of the given-y sweep.
    python tools/time_nested_phantoms.py stats [--seeds 8] [--json out.json]
        the Gaussian in [-4, 4]^d fitted by a surrogate (d = 2 and 5): plain against merged logZ, posterior mean, ESS.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _bench_model():
    import bench
    N, d, M = 4096, 16, 1000
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    return gpr, np.asarray(bounds, dtype=float)


def _ess(w):
    return float(1.0 / np.sum(np.asarray(w) ** 2))


def _first_generation(gpr, bounds, seed, nlive=400, nprior=4000):
    from gpry_amd.nested import whitening
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
    X, y, _ = gpr.device.ns_prior(lo, hi, seed, nprior)
    order = np.lexsort((np.arange(nprior), y))
    k = nlive // 2
    keep = np.sort(order[nprior - nlive + k:])
    Xs, ys = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
    lstar = float(y[order[nprior - nlive + k - 1]])
    return lo, hi, Xs, ys, lstar, whitening((Xs - lo) / (hi - lo)), k


def cmd_gen(args):
    gpr, bounds = _bench_model()
    dev = gpr.device
    lo, hi, Xs, ys, lstar, W, k = _first_generation(gpr, bounds, 100)
    R = 5 * len(lo)
    variants = {"plain": lambda: dev.ns_generation(lo, hi, Xs, ys, lstar, W, 100, 0, k, R)}
    if not args.plain_only:
        for thin in (1, 2, 5):
            variants[f"thin {thin}"] = (lambda t: lambda: dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 100, 0, k,
                                                                                    R, t))(thin)
    times = {name: [] for name in variants}
    for rep in range(args.reps + 1):
        for name, call in variants.items():
            t0 = time.perf_counter()
            out = call()
            wall = time.perf_counter() - t0
            if rep:
                times[name].append((out[-1], wall * 1e3, int(np.sum(out[2]))))
    res = {"N": gpr.n, "d": len(lo), "k": k, "num_repeats": R, "device": dev.info()["arch"], "variants": {}}
    for name, rows in times.items():
        dm, wm = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        res["variants"][name] = dict(device_ms_median=float(np.median(dm)), device_ms_min=float(dm.min()),
                                     device_ms_max=float(dm.max()), wall_ms_median=float(np.median(wm)),
                                     evaluations=rows[0][2])
        print(f"{name:8s}: device {np.median(dm):8.3f} ms (min {dm.min():.3f}, max {dm.max():.3f}), wall "
              f"{np.median(wm):8.3f} ms, {rows[0][2]} evaluations")
    return res


def cmd_runs(args):
    from gpry_amd import nested
    from gpry_amd.gp_acquisition import NORA
    gpr, bounds = _bench_model()
    acq = NORA(bounds, sampler="nested", verbose=0, devices=[0])
    prec = acq.update_NS_precision(gpr)
    host = []
    real = nested.merged_weights

    def timed(*a, **kw):
        t0 = time.perf_counter()
        out = real(*a, **kw)
        host.append((time.perf_counter() - t0, len(a[0])))
        return out

    nested.merged_weights = timed
    res = {"settings": prec, "runs": {}}
    for seed in range(args.runs + 1):
        for thin in (None, 1, 2, 5):
            del host[:]
            r = nested.run_nested(gpr.device, bounds, 100 + seed, prec["nlive"], prec["num_repeats"],
                                  precision_criterion=prec["precision_criterion"], nprior=prec["nprior"],
                                  max_ncalls=prec["max_ncalls"], minus_inf_value=gpr.minus_inf_value,
                                  **({} if thin is None else {"phantom_thin": thin}))
            if seed == 0:
                continue                      # (the first round loads the code objects)
            row = dict(seed=100 + seed, rows=len(r.y), ess=_ess(r.w), device_s=r.device_s, wall_s=r.wall_s,
                       ncalls=r.ncalls, generations=r.ngen, logZ=r.logZ, logZ_err=r.logZ_err,
                       logZ_merged=r.logZ_merged, merged_weights_ms=host[0][0] * 1e3 if host else None,
                       merged_points=host[0][1] if host else None)
            res["runs"].setdefault(str(thin), []).append(row)
            print(f"thin {thin}: {row}")
    nested.merged_weights = real
    res["multi_add"] = {}
    for thin in (None, 1, 2, 5):
        a = NORA(bounds, sampler="nested", verbose=0, devices=[0], nested_phantoms=thin)
        a.multi_add(gpr, n_points=4, rng=np.random.default_rng(0))          # warm-up of this pool size
        a = NORA(bounds, sampler="nested", verbose=0, devices=[0], nested_phantoms=thin)
        t0 = time.perf_counter()
        a.multi_add(gpr, n_points=4, rng=np.random.default_rng(1))
        row = dict(multi_add_s=time.perf_counter() - t0, sweep_s=a.stats["sweep_s"], sweep_M=a.stats["sweep_M"],
                   sampler_info=a.stats["sampler_info"])
        res["multi_add"][str(thin)] = row
        print(f"multi_add thin {thin}: {row}")
    return res


def cmd_stats(args):
    from oracle import gpry_oracle as orc
    from test_host_mirror_gpu import make_gpr
    from gpry_amd.nested import run_nested
    res = {}
    for d, thin in ((2, 1), (5, 2)):
        rng = np.random.default_rng(d)
        N = 150 * d
        X = np.concatenate([rng.uniform(-4, 4, (N // 2, d)), np.clip(0.3 + rng.normal(0, 0.7, (N - N // 2, d)), -4, 4)])
        y = -0.5 * np.sum((X - 0.3) ** 2, axis=1) / 0.25 - 0.5 * d * np.log(2 * np.pi * 0.25)
        bounds = np.array([[-4.0, 4.0]] * d)
        gpr = make_gpr(bounds, orc.MATERN52, n_restarts_optimizer=1, random_state=1)
        gpr.append_to_data(X, y, fit_gpr=True)
        gpr._ensure_factor()
        gpr._push_affine()
        assert gpr._push_gates()
        # the surrogate's own evidence and mean from a long plain run
        ref = run_nested(gpr.device, bounds, 999, 100 * d, 5 * d, nprior=1000 * d, minus_inf_value=gpr.minus_inf_value)
        ref_mean = ref.w @ ref.X
        rows = []
        for seed in range(1, args.seeds + 1):
            kw = dict(nprior=250 * d, minus_inf_value=gpr.minus_inf_value)
            a = run_nested(gpr.device, bounds, seed, 25 * d, 5 * d, **kw)
            b = run_nested(gpr.device, bounds, seed, 25 * d, 5 * d, phantom_thin=thin, **kw)
            assert a.logZ == b.logZ and a.ncalls == b.ncalls
            rows.append(dict(seed=seed, rows=(len(a.y), len(b.y)), ess=(_ess(a.w), _ess(b.w)), logZ=a.logZ,
                             logZ_merged=b.logZ_merged, logZ_err=a.logZ_err,
                             mean_err=(float(np.sqrt(np.mean((a.w @ a.X - ref_mean) ** 2))),
                                       float(np.sqrt(np.mean((b.w @ b.X - ref_mean) ** 2))))))
        rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
        summary = dict(d=d, thin=thin, ref_logZ=ref.logZ, ref_logZ_err=ref.logZ_err,
                       rows=(float(np.mean([r["rows"][0] for r in rows])), float(np.mean([r["rows"][1] for r in rows]))),
                       ess=(float(np.mean([r["ess"][0] for r in rows])), float(np.mean([r["ess"][1] for r in rows]))),
                       rms_logZ=(rms([r["logZ"] - ref.logZ for r in rows]), rms([r["logZ_merged"] - ref.logZ for r in rows])),
                       rms_mean=(rms([r["mean_err"][0] for r in rows]), rms([r["mean_err"][1] for r in rows])),
                       worst_logZ_merged=float(np.max([abs(r["logZ_merged"] - ref.logZ) for r in rows])),
                       logZ_err=float(np.mean([r["logZ_err"] for r in rows])))
        print(summary)
        res[f"d={d}"] = dict(summary=summary, all=rows)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gen", "runs", "stats"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {"gen": cmd_gen, "runs": cmd_runs, "stats": cmd_stats}[args.what](args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, default=float)


if __name__ == "__main__":
    main()
