"""Metropolis MCMC of the surrogate on the device, on the bench's fitted model (BASELINE configs[2]: N = 4096, d = 16):
evaluations per second against the number of chains, mapped pinned output against device buffers copied back once,
full run_mcmc runs to R - 1 < 0.01 (wall, evaluations, acceptance) for a few settings of the adaptation, and the same
work priced at the one-point gpr.predict rate measured in the same process.  Writes a JSON file and a markdown table.

    python tools/time_mcmc.py [--json profiles/mcmc.json] [--md profiles/mcmc.md] [--max-ncalls 2e8]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _rate(dev, bounds, X0, Lp, nsteps, thin, reps=3):
    """Median over reps of one call: device ms, wall ms, evaluations."""
    lo, hi = bounds[:, 0], bounds[:, 1]
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        out = dev.mcmc_chains(lo, hi, X0, np.full(len(X0), np.nan), Lp, 1.0, -np.inf, 7, r, nsteps, thin)
        wall = time.perf_counter() - t0
        if r:
            rows.append((out["device_ms"], wall * 1e3, int(np.sum(out["ncalls"])), float(np.mean(out["naccept"])) / nsteps))
    dms, wms, ev, acc = (float(np.median([row[k] for row in rows])) for k in range(4))
    return dict(device_ms=dms, wall_ms=wms, evals=ev, evals_per_s_device=ev / dms * 1e3, evals_per_s_wall=ev / wms * 1e3,
                acceptance=acc, record_MB=len(X0) * (nsteps // thin) * (X0.shape[1] + 1) * 8 / 2**20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--max-ncalls", type=float, default=2e8)
    args = ap.parse_args()
    import bench
    from gpry_amd.mcmc import PROPOSAL_SCALE, _weighted_cov, run_mcmc
    from gpry_amd.nested import cholesky_ridged
    N, d, M = 4096, 16, 1000
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = "?"
    out = {"N": gpr.n, "d": d, "device": gpr.device.info()["arch"], "build": (rev or "?") + " + working tree"}
    for x in Xc[:50]:
        gpr.predict(x[None, :], validate=False)
    t0 = time.perf_counter()
    for x in Xc[:1000]:
        gpr.predict(x[None, :], validate=False)
    t_pt = (time.perf_counter() - t0) / 1000
    out["predict_one_point_us"] = t_pt * 1e6
    print(f"one-point gpr.predict: {t_pt * 1e6:.2f} us per call = {1 / t_pt:.3g} evaluations/s", flush=True)
    dev = gpr.device
    span = bounds[:, 1] - bounds[:, 0]
    Lp = PROPOSAL_SCALE / np.sqrt(d) * cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))
    rng = np.random.default_rng(0)
    # ---- rate against the number of chains (device buffers, the default), 200 steps per call, every state recorded
    out["chains"] = {}
    for n in (64, 128, 256, 512, 1024):
        X0 = np.ascontiguousarray(gpr.X_train[rng.choice(gpr.n, n)])
        r = _rate(dev, bounds, X0, Lp, 200, 1)
        out["chains"][str(n)] = r
        print(f"nchains {n:5d}: {r['evals_per_s_device']:.3g} evaluations/s device, {r['evals_per_s_wall']:.3g} wall "
              f"({r['device_ms']:.2f} ms / call, {r['record_MB']:.1f} MB of records)", flush=True)
    # ---- mapped pinned output against device buffers
    out["memory_path"] = {}
    for n in (256, 1024):
        X0 = np.ascontiguousarray(gpr.X_train[rng.choice(gpr.n, n)])
        for mapped in (0, 1):
            dev.set_option("mcmc_mapped", mapped)
            r = _rate(dev, bounds, X0, Lp, 200, 1)
            out["memory_path"][f"{n} {'mapped' if mapped else 'device'}"] = r
            print(f"nchains {n:5d} {'mapped' if mapped else 'device'}: device {r['device_ms']:.2f} ms, wall "
                  f"{r['wall_ms']:.2f} ms, {r['record_MB']:.1f} MB", flush=True)
        dev.set_option("mcmc_mapped", 0)
    # ---- full runs to R - 1 < 0.01
    out["runs"] = {}
    settings = [dict(nchains=256, learn_every=100, learn_batches=4), dict(nchains=512, learn_every=100, learn_batches=4),
                dict(nchains=1024, learn_every=100, learn_batches=4), dict(nchains=256, learn_every=50, learn_batches=2),
                dict(nchains=256, learn_every=200, learn_batches=4), dict(nchains=512, learn_every=200, learn_batches=4)]
    run_mcmc(dev, bounds, 99, 256, gpr.X_train, gpr.y_train, max_batches=2, minus_inf_value=gpr.minus_inf_value)  # warm-up
    for s in settings:
        r = run_mcmc(dev, bounds, 1, s["nchains"], gpr.X_train, gpr.y_train, learn_every=s["learn_every"],
                     learn_batches=s["learn_batches"], max_ncalls=int(args.max_ncalls),
                     minus_inf_value=gpr.minus_inf_value)
        key = f"nchains={s['nchains']} learn_every={s['learn_every']} learn_batches={s['learn_batches']}"
        row = dict(wall_s=r.wall_s, device_s=r.device_s, ncalls=r.ncalls, evals_per_s=r.ncalls / r.device_s,
                   acceptance=r.acceptance, batches=r.batches, converged=r.converged, Rminus1=float(r.Rminus1[-1]),
                   rows=len(r.y), one_point_s=r.ncalls * t_pt)
        out["runs"][key] = row
        print(f"{key}: wall {r.wall_s:.2f} s, device {r.device_s:.2f} s, {r.ncalls:.3g} evaluations, acceptance "
              f"{r.acceptance:.3f}, {r.batches} batches, R-1 {row['Rminus1']:.4f}, converged {r.converged}, {len(r.y)} rows; "
              f"at the one-point rate {row['one_point_s']:.0f} s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1, default=float)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def markdown(out):
    L = [f"Measured by `python tools/time_mcmc.py`, one {out['device']}, build {out['build']}; model: the bench's fitted "
         f"model (N = {out['N']}, d = {out['d']}).  One-point `gpr.predict`: {out['predict_one_point_us']:.2f} µs per call.",
         "", "| chains | device ms / call (200 steps) | evaluations / s (device) | evaluations / s (wall) | records |",
         "|---|---|---|---|---|"]
    for n, r in out["chains"].items():
        L.append(f"| {n} | {r['device_ms']:.2f} | {r['evals_per_s_device']:.3g} | {r['evals_per_s_wall']:.3g} | "
                 f"{r['record_MB']:.1f} MB |")
    L += ["", "| chains, output | device ms | wall ms |", "|---|---|---|"]
    for k, r in out["memory_path"].items():
        L.append(f"| {k} | {r['device_ms']:.2f} | {r['wall_ms']:.2f} |")
    L += ["", "| run_mcmc setting | wall s | device s | evaluations | evaluations / s | acceptance | batches | R - 1 | "
          "converged | rows | at one-point predict |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for k, r in out["runs"].items():
        L.append(f"| {k} | {r['wall_s']:.2f} | {r['device_s']:.2f} | {r['ncalls']:.3g} | {r['evals_per_s']:.3g} | "
                 f"{r['acceptance']:.3f} | {r['batches']} | {r['Rminus1']:.4f} | {r['converged']} | {r['rows']} | "
                 f"{r['one_point_s']:.0f} s |")
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
