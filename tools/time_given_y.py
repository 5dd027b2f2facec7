"""Wall time of `sweep + sweep_topk(256)` at BASELINE configs[2] (N = 4096, d = 16, M = 1e6) for the sweeps of a pool whose
sampler supplied y (gpry_sweep_logexp_given) against the ordinary pruned sweep, on the bench's fitted model and on
theta = log[4, 0.3...].  The pool is resident (X = None), as in NORA's own sweep of a re-used sample.

    python tools/time_given_y.py [--reps 5] [--json out.json]

Variants: ordinary pruned (option "sweep_prune", y computed), sigma-only pruned, sigma-only full, both given.  The caller's
y is the ordinary sweep's own, so every variant selects the same shortlist (checked)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def models(N, d, M):
    import bench
    from oracle import gpry_oracle as orc
    from test_host_mirror_gpu import make_gpr
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    yield "bench fitted model", gpr, Xc
    bounds, X, y, Xc = orc.synthetic_problem(N, d, M)
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.log(np.array([4.0] + [0.3] * d)))
    gpr.append_to_data(X, y, fit_gpr=False)
    yield "theta = log[4, 0.3...]", gpr, Xc


def run(gpr, Xc, reps, only=None):
    from oracle import gpry_oracle as orc
    gpr._ensure_factor()
    gpr._push_affine()
    dev = gpr.device
    zeta, base, sn, M = orc.auto_zeta(gpr.d), gpr.y_max, gpr.noise_level, len(Xc)
    full = dev.sweep_logexp(Xc, zeta, base, sn)            # uploads the pool; the sweep's own y and sigma
    ref, _ = dev.sweep_topk(256)
    yg, sg = full["y"], full["sigma"]
    variants = {
        "ordinary pruned": (1, {}),
        "sigma-only pruned": (1, {"y_given": yg}),
        "sigma-only full": (0, {"y_given": yg}),
        "both given": (0, {"y_given": yg, "sigma_given": sg}),
    }
    res = {}
    for name, (prune, kw) in variants.items():
        if only and name != only:
            continue
        ts, info = [], None
        for r in range(reps + 1):
            dev.set_option("sweep_prune", prune)
            try:
                t0 = time.perf_counter()
                dev.sweep_logexp(None, zeta, base, sn, M=M, want=(), **kw)
                top, _ = dev.sweep_topk(256)
                t = time.perf_counter() - t0
            finally:
                dev.set_option("sweep_prune", 0)
            if r:                                           # (the first call is a warm-up)
                ts.append(t * 1e3)
            info = dev.sweep_prune_info() if prune else None
            assert np.array_equal(top["idx"], ref["idx"]) and np.array_equal(top["acq"], ref["acq"]), name
        res[name] = {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "reps": reps,
                     "contracted": None if info is None else info["contracted"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="one variant (e.g. 'sigma-only pruned'), for a profiler run")
    ap.add_argument("--model", type=int, default=None, help="0: the bench's fitted model, 1: theta = log[4, 0.3...]")
    a = ap.parse_args()
    out = {}
    for i, (label, gpr, Xc) in enumerate(models(4096, 16, 1_000_000)):
        if a.model is not None and i != a.model:
            continue
        out[label] = run(gpr, Xc, a.reps, a.only)
        for name, r in out[label].items():
            print(f"{label:24s} {name:20s} median {r['ms_median']:8.2f} ms  min {r['ms_min']:8.2f} ms  "
                  f"contracted {r['contracted']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
