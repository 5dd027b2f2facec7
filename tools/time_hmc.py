"""HMC against Metropolis MCMC of the surrogate on the device, from fixed seeds, on three models: the bench's fitted model
(BASELINE configs[2]: 4080 training rows, d = 16) and peaked Gaussian surrogates at d = 16 and d = 30 (2000 training points,
Matern-5/2, fixed hyper-parameters).  Per model: run_mcmc at its defaults, run_hmc at its defaults and run_hmc with
reflect=True (the row hmc-reflect, with its reflections per trajectory) to R - 1 < 0.01 (evaluations = mean + gradient, wall
seconds, acceptance, eps, nleap, the effective sample size of the slowest coordinate per 1e6 evaluations and per second);
on the bench's model also the device time per trajectory at 256 / 512 / 1024 chains; on peaked16 the cost of the
reflection flag where no wall is touched: device ms per trajectory of 256 chains with reflect on and off, calls
alternating, medians over 2 x reps + 1 calls of 100 trajectories each.  Warm context (one short run of each sampler first), medians over --reps runs.  Writes a JSON file and a markdown table.

    python tools/time_hmc.py [--json profiles/hmc.json] [--md profiles/hmc_tables.md] [--reps 3] [--max-ncalls 6e7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def ess_slowest(X, nchains):
    """Effective sample size of the slowest coordinate, from the scatter of the chains' means: m sigma^2 / var(means)."""
    d = X.shape[1]
    Xc = X.reshape(nchains, -1, d)
    return float(np.min(nchains * X.var(axis=0) / Xc.mean(axis=1).var(axis=0, ddof=1)))


def peaked(d, N=2000, seed=0):
    """Surrogate of N(0.3, 0.5^2 I) on [-4, 4]^d."""
    from test_host_mirror_gpu import make_gpr
    rng = np.random.default_rng(seed)
    X = np.clip(np.concatenate([rng.normal(0.3, 0.8, (N - N // 8, d)), rng.uniform(-4, 4, (N // 8, d))]), -4, 4)
    y = -0.5 * np.sum((X - 0.3) ** 2, axis=1) / 0.25
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = make_gpr(bounds, 3, theta=np.log([100.0] + [1.0] * d))
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


def one(run, reps):
    rows = [run(seed) for seed in range(1, reps + 1)]
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    med["converged"] = all(r["converged"] for r in rows)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-ncalls", type=float, default=6e7)
    ap.add_argument("--models", default="bench,peaked16,peaked30")
    args = ap.parse_args()
    import bench
    from gpry_amd.hmc import DEFAULT_BATCH_STEPS, DEFAULT_LEARN_BATCHES, DEFAULT_LEARN_EVERY, leapfrog_steps, run_hmc
    from gpry_amd.mcmc import _weighted_cov, run_mcmc
    from gpry_amd.nested import cholesky_ridged
    out = {"models": {}, "reps": args.reps}
    for name in args.models.split(","):
        if name == "bench":
            bounds, X, y, _, _ = bench.synthetic(4096 - 16, 16, 1000)
            gpr = bench.make_gpr(bounds)
            gpr.append_to_data(X, y, fit_gpr="simple")
        else:
            gpr, bounds = peaked(int(name[6:]))
        gpr._ensure_factor()
        gpr._push_affine()
        assert gpr._push_gates()
        dev, d = gpr.device, len(bounds)
        out["device"] = dev.info()["arch"]
        kw = dict(minus_inf_value=gpr.minus_inf_value)
        run_mcmc(dev, bounds, 99, 256, gpr.X_train, gpr.y_train, max_batches=2, **kw)          # warm-up
        run_hmc(dev, bounds, 99, 256, gpr.X_train, gpr.y_train, max_batches=2, **kw)

        def mcmc(seed):
            r = run_mcmc(dev, bounds, seed, 256, gpr.X_train, gpr.y_train, max_ncalls=int(args.max_ncalls), **kw)
            ess = ess_slowest(r.X, 256)
            return dict(evals=r.ncalls, wall_s=r.wall_s, device_s=r.device_s, acceptance=r.acceptance, ess=ess,
                        ess_per_1e6=ess / r.ncalls * 1e6, ess_per_s=ess / r.wall_s, converged=r.converged,
                        Rminus1=float(r.Rminus1[-1]))

        def hmc(seed, **own):
            r = run_hmc(dev, bounds, seed, 256, gpr.X_train, gpr.y_train, max_ncalls=int(args.max_ncalls), **own, **kw)
            ess, ev = ess_slowest(r.X, 256), r.ncalls + r.ngrad
            ntraj = 256 * (DEFAULT_LEARN_BATCHES * DEFAULT_LEARN_EVERY + r.batches * DEFAULT_BATCH_STEPS)
            return dict(evals=ev, wall_s=r.wall_s, device_s=r.device_s, acceptance=r.acceptance, ess=ess,
                        ess_per_1e6=ess / ev * 1e6, ess_per_s=ess / r.wall_s, converged=r.converged,
                        Rminus1=float(r.Rminus1[-1]), eps=r.eps, nleap=r.nleap, reflections=r.nreflect / ntraj)

        def hmc_reflect(seed):
            return hmc(seed, reflect=True)

        m = {"N": gpr.n, "d": d, "mcmc": one(mcmc, args.reps), "hmc": one(hmc, args.reps),
             "hmc-reflect": one(hmc_reflect, args.reps)}
        print(name, json.dumps(m, default=float), flush=True)
        if name == "bench":
            # device time per trajectory against the number of chains, at the adapted eps / nleap of the runs above
            span = bounds[:, 1] - bounds[:, 0]
            Lp = cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))
            eps = m["hmc"]["eps"]
            nleap = leapfrog_steps(eps)
            rng = np.random.default_rng(0)
            m["chains"] = {}
            for n in (256, 512, 1024):
                X0 = np.ascontiguousarray(gpr.X_train[rng.choice(gpr.n, n)])
                ms, gr = [], []
                for r in range(args.reps + 1):
                    o = dev.hmc_chains(bounds[:, 0], bounds[:, 1], X0, np.full(n, np.nan), Lp, eps, nleap, 1.0, -np.inf, 7, r,
                                       20, 1)
                    if r:
                        ms.append(o["device_ms"] / 20)
                        gr.append(float(np.sum(o["ngrad"] + o["ncalls"])) / o["device_ms"] * 1e3)
                m["chains"][str(n)] = dict(ms_per_trajectory=float(np.median(ms)), evals_per_s=float(np.median(gr)),
                                           nleap=nleap, eps=eps)
                print(f"nchains {n}: {np.median(ms):.3f} ms per trajectory of all chains (nleap = {nleap}), "
                      f"{np.median(gr):.3g} evaluations/s", flush=True)
        if name == "peaked16":
            # the cost of the flag where no wall is touched: the same call with reflect off and on, alternating
            span = bounds[:, 1] - bounds[:, 0]
            Lp = cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))
            eps = m["hmc"]["eps"]
            nleap = leapfrog_steps(eps)
            X0 = np.ascontiguousarray(gpr.X_train[np.random.default_rng(0).choice(gpr.n, 256)])
            ms, nrefl = {False: [], True: []}, 0
            for r in range(2 * (2 * args.reps + 2)):
                rf = bool(r % 2)
                o = dev.hmc_chains(bounds[:, 0], bounds[:, 1], X0, np.full(256, np.nan), Lp, eps, nleap, 1.0, -np.inf, 7,
                                   r // 2, 100, 1, **(dict(reflect=True) if rf else {}))
                if r >= 2:                          # (the first call of each is the warm-up)
                    ms[rf].append(o["device_ms"] / 100)
                    nrefl += int(np.sum(o.get("nreflect", 0)))
            m["flag"] = dict(ms_per_trajectory_off=float(np.median(ms[False])), ms_per_trajectory_on=float(np.median(ms[True])),
                             off=ms[False], on=ms[True], nleap=nleap, eps=eps, reflections=nrefl)
            print(f"flag on peaked16: {np.median(ms[False]):.4f} ms per trajectory of 256 chains with reflect off "
                  f"({min(ms[False]):.4f} .. {max(ms[False]):.4f}), {np.median(ms[True]):.4f} on ({min(ms[True]):.4f} .. "
                  f"{max(ms[True]):.4f}); {nrefl} reflections", flush=True)
        out["models"][name] = m
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1, default=float)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def _num(v, fmt):
    return "–" if v != v else format(v, fmt)


def markdown(out):
    L = [f"Measured by `python tools/time_hmc.py --reps {out['reps']}`, one {out.get('device', '?')}; medians over seeds "
         f"1..{out['reps']}, 256 chains, warm context.", "",
         "| model | sampler | evaluations | wall s | device s | acceptance | eps | nleap | ESS slowest | ESS / 1e6 evaluations | "
         "ESS / s | R - 1 | converged | reflections / trajectory |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, m in out["models"].items():
        for s in ("mcmc", "hmc", "hmc-reflect"):
            r = m[s]
            L.append(f"| {name} (N = {m['N']}, d = {m['d']}) | {s} | {r['evals']:.3g} | {r['wall_s']:.2f} | {r['device_s']:.2f} | "
                     f"{r['acceptance']:.3f} | {_num(r.get('eps', float('nan')), '.3f')} | {_num(r.get('nleap', float('nan')), '.0f')} | "
                     f"{r['ess']:.3g} | {r['ess_per_1e6']:.3g} | {r['ess_per_s']:.3g} | {r['Rminus1']:.4f} | {r['converged']} | "
                     f"{_num(r.get('reflections', float('nan')), '.2f')} |")
    for name, m in out["models"].items():
        if "chains" in m:
            L += ["", f"| chains ({name}) | device ms per trajectory | evaluations / s | nleap |", "|---|---|---|---|"]
            for n, r in m["chains"].items():
                L.append(f"| {n} | {r['ms_per_trajectory']:.3f} | {r['evals_per_s']:.3g} | {r['nleap']} |")
    for name, m in out["models"].items():
        if "flag" in m:
            r = m["flag"]
            L += ["", f"| reflect ({name}, 256 chains, nleap = {r['nleap']}) | device ms per trajectory | range |", "|---|---|---|",
                  f"| off | {r['ms_per_trajectory_off']:.4f} | {min(r['off']):.4f} .. {max(r['off']):.4f} |",
                  f"| on ({r['reflections']} reflections) | {r['ms_per_trajectory_on']:.4f} | {min(r['on']):.4f} .. "
                  f"{max(r['on']):.4f} |"]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
