"""Tempered Metropolis ladders on the device (gpry_mcmc_ladders) against the plain chains (gpry_mcmc_chains), in one
process on one build.  On the bench's fitted model (BASELINE configs[2]: N = 4096, d = 16): evaluations per second of 256
ladders of 2 / 4 / 8 rungs and of 256 and 256 R plain chains, 200 steps per call, device_ms from the HIP events, median
of the calls after a warm-up one; full runs of run_tempered against run_mcmc there and on the two-mode mixture surrogate
of tests/test_mcmc_ladders_gpu.py.  Writes a JSON file.

    python tools/time_mcmc_ladders.py [--json out.json] [--reps 7] [--max-ncalls 3e7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _median_call(call, reps):
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        out = call(r)
        wall = time.perf_counter() - t0
        if r:
            rows.append((out["device_ms"], wall * 1e3, int(np.sum(out["ncalls"]))))
    dms, wms, ev = (float(np.median([row[k] for row in rows])) for k in range(3))
    return dict(device_ms=dms, wall_ms=wms, evals=ev, evals_per_s_device=ev / dms * 1e3, evals_per_s_wall=ev / wms * 1e3,
                device_ms_all=[row[0] for row in rows])


def _run_row(r):
    row = dict(wall_s=r.wall_s, device_s=r.device_s, ncalls=r.ncalls, batches=r.batches, converged=bool(r.converged),
               Rminus1=float(r.Rminus1[-1]), rows=len(r.y), acceptance=r.acceptance)
    if hasattr(r, "swap_acceptance"):
        row.update(acceptance_per_rung=list(map(float, r.acceptance_per_rung)), temperatures=list(map(float, r.temperatures)),
                   swap_acceptance=list(map(float, r.swap_acceptance)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-ncalls", type=float, default=3e7)
    args = ap.parse_args()
    import bench
    from gpry_amd.mcmc import PROPOSAL_SCALE, _weighted_cov, run_mcmc
    from gpry_amd.nested import cholesky_ridged
    from gpry_amd.tempering import ladder, run_tempered
    N, d, M = 4096, 16, 1000
    bounds, X, y, _, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    dev = gpr.device
    out = {"N": gpr.n, "d": d, "device": dev.info()["arch"]}
    lo, hi = bounds[:, 0], bounds[:, 1]
    span = hi - lo
    L0 = PROPOSAL_SCALE / np.sqrt(d) * cholesky_ridged(_weighted_cov(gpr.X_train, gpr.y_train) / np.outer(span, span))
    rng = np.random.default_rng(0)
    X0 = np.ascontiguousarray(gpr.X_train[rng.choice(gpr.n, 256 * 8)])
    nan = np.full(len(X0), np.nan)
    # ---- rate: ladders of R against plain chains of equal count, 200 steps per call, every state recorded
    out["rate"] = {}
    for n in (256, 512, 1024, 2048):
        r = _median_call(lambda b: dev.mcmc_chains(lo, hi, X0[:n], nan[:n], L0, 1.0, -np.inf, 7, b, 200, 1), args.reps)
        out["rate"][f"plain {n}"] = r
        print(f"plain chains {n:5d}: {r['evals_per_s_device']:.3g} evaluations/s device ({r['device_ms']:.2f} ms / call)",
              flush=True)
    for R in (2, 4, 8):
        T = ladder(d, rungs=R)
        for name, TT in (("equal T", np.ones(R)), ("ladder T", T)):
            # equal T: the chains of the plain rows, packed R to a workgroup; ladder T: the default ladder, wider hot rungs
            Lp = np.array([L0 * np.sqrt(t) for t in TT])
            for se in (0, 5):
                r = _median_call(lambda b: dev.mcmc_ladders(lo, hi, X0[:256 * R], nan[:256 * R], R, Lp, TT, -np.inf, 7, b,
                                                            200, 1, se), args.reps)
                out["rate"][f"ladders 256 x {R}, {name}, swap_every {se}"] = r
                print(f"ladders 256 x {R} ({name}, swap_every {se}): {r['evals_per_s_device']:.3g} evaluations/s device "
                      f"({r['device_ms']:.2f} ms / call, {r['evals']:.0f} evaluations)", flush=True)
    # ---- full runs
    out["runs"] = {}
    kw = dict(max_ncalls=int(args.max_ncalls), minus_inf_value=gpr.minus_inf_value)
    run_mcmc(dev, bounds, 99, 256, gpr.X_train, gpr.y_train, max_batches=2, minus_inf_value=gpr.minus_inf_value)    # warm-up
    out["runs"]["bench model, run_mcmc 256 chains"] = _run_row(run_mcmc(dev, bounds, 1, 256, gpr.X_train, gpr.y_train, **kw))
    out["runs"]["bench model, run_tempered 64 ladders x 6"] = _run_row(run_tempered(dev, bounds, 1, 64, gpr.X_train,
                                                                                    gpr.y_train, **kw))
    from test_mcmc_ladders_gpu import _mixture_model, _mode_1
    gm, bm = _mixture_model()
    gm._ensure_factor()
    gm._push_affine()
    assert gm._push_gates()
    kw = dict(max_ncalls=int(args.max_ncalls) // 8, minus_inf_value=gm.minus_inf_value)    # (run_mcmc never converges there)
    for name, r in (("mixture, run_mcmc 256 chains", run_mcmc(gm.device, bm, 1, 256, gm.X_train, gm.y_train, **kw)),
                    ("mixture, run_tempered 64 ladders x 6", run_tempered(gm.device, bm, 1, 64, gm.X_train, gm.y_train, **kw))):
        row = _run_row(r)
        row["mass_mode_1"] = float(np.sum(r.w[_mode_1(r.X)]))
        out["runs"][name] = row
    for k, row in out["runs"].items():
        print(k, json.dumps(row, default=float), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1, default=float)


if __name__ == "__main__":
    main()
