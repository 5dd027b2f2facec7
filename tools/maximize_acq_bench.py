"""Measurements behind profiles/maximize_acq.md: ``BatchOptimizer.multi_add(n_points=4)`` with the acquisition maximised on
the device (``acq_optimizer="device"``, gpry_maximize_acq) against the side-by-side L-BFGS-B path
(``acq_optimizer="fmin_l_bfgs_b"``, ``lockstep="auto"``), and the time of one evaluation inside the kernel.

    python tools/maximize_acq_bench.py [--out profiles/maximize_acq.md] [--sizes 256,1024,2048,4092]

Every size runs in a child process of its own (``--child N``) under a time limit; a child that fails, or runs into its
limit, ends the run: nothing more is started on the GPU after it.  d = 8, RBF, the default 5d = 40 restarts; medians of
5 calls after one warm-up.  The largest size is 4092 and not 4096: the three lies of a call with n_points = 4 are
border rows, and the kernel takes models of at most 4096 padded rows."""
import argparse
import json
import os
import subprocess
import sys
from time import perf_counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, N_POINTS, REPEATS, CHILD_LIMIT_S = 8, 4, 5, 420


def model(N, d=D, seed=0):
    """A Gaussian log-likelihood (sigma 1.5) on [-4, 4]^d, half of the rows uniform, half around the mode; RBF with
    length scales of 0.45 of the box, C = 4, noise 0.1, y not normalised."""
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import clone
    from gpry_amd.preprocessing import Normalize_bounds
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-4, 4, (N // 2, d)), np.clip(rng.normal(0.0, 1.0, (N - N // 2, d)), -4, 4)])
    y = -0.5 * np.sum((X - 0.3) ** 2, axis=1) / 1.5 ** 2
    bounds = np.array([[-4.0, 4.0]] * d)
    gpr = GaussianProcessRegressor(kernel="RBF", bounds=bounds, preprocessing_X=Normalize_bounds(bounds), preprocessing_y=None,
                                   account_for_inf=None, noise_level=0.1)
    k = clone(gpr.kernel)
    k.theta = np.log([4.0] + [0.45] * d)
    gpr.kernel_, gpr._fitted = k, True
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


def child(N):
    from gpry_amd.acquisition_functions import LogExp
    from gpry_amd.gp_acquisition import BatchOptimizer
    from gpry_amd.maximize import MAX_STATUS, maximize_acq
    gpr, bounds = model(N)
    lo, hi = bounds[:, 0].copy(), bounds[:, 1].copy()
    out = {"N": N, "Np": -(-N // 128) * 128}
    # ---- the kernel alone: 40 uniform starts, the controls of the optimiser path
    maximize_acq(gpr, nstarts=40, rng=1)
    r = maximize_acq(gpr, nstarts=40, rng=1)
    evals = int(np.sum(r.ncalls + r.ngrad))
    out.update(kernel_ms=1e3 * r.device_s, kernel_evals=evals, per_eval_us=1e6 * r.device_s * 40 / evals,
               status={MAX_STATUS[k]: int(v) for k, v in enumerate(np.bincount(r.status, minlength=6))},
               iters=[int(v) for v in np.quantile(r.iters, [0, 0.25, 0.5, 0.75, 1.0])],
               v_mb=8.0 * N * (N + 1) / 2 / 1e6)
    # ---- the gradient against the one-point predict (y_std = 1 here, so that predict's std_grad is d sigma / dx)
    zeta, sn = float(LogExp(dimension=D).zeta), 0.1
    X = np.ascontiguousarray(np.random.default_rng(2).uniform(lo, hi, (24, D)))
    g = gpr.device.maximize_acq(lo, hi, X, np.zeros(D, bool), np.eye(D), zeta, float(gpr.y_max), sn, 0, 0, 1e-6, 0.0, -np.inf)
    ref = np.full((24, D), np.nan)
    for p, x in enumerate(X):
        _, sd, mg, sg = gpr.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True)
        if sd[0] ** 2 - sn ** 2 >= 0.04:
            ref[p] = (hi - lo) / 8.0 * (2 * zeta * np.ravel(mg) + sd[0] * np.ravel(sg) / (sd[0] ** 2 - sn ** 2))
    ok = np.isfinite(ref[:, 0])
    out["grad_rows"] = int(ok.sum())
    out["grad_err"] = float(np.max(np.abs(g["G"][ok] - ref[ok])) / np.max(np.abs(ref[ok]))) if ok.any() else None
    # ---- multi_add, both optimisers
    for opt in ("device", "fmin_l_bfgs_b"):
        acq = BatchOptimizer(bounds, acq_optimizer=opt, verbose=0)
        times = []
        for rep in range(REPEATS + 1):
            t0 = perf_counter()
            Xo, yl, av = acq.multi_add(gpr, n_points=N_POINTS, rng=np.random.default_rng(5))
            times.append(perf_counter() - t0)
        out[opt] = dict(ms=1e3 * float(np.median(times[1:])), all_ms=[round(1e3 * t, 1) for t in times[1:]],
                        acq=[float(v) for v in av], stats={k: v for k, v in acq.stats.items() if k != "prune"})
    print("RESULT " + json.dumps(out), flush=True)


def table(rows):
    L = ["# Maximisation of the LogExp acquisition on the device: measurements", "",
         "Written by `tools/maximize_acq_bench.py` on one MI355X; d = 8, RBF, 40 restarts per proposal, `multi_add(n_points=4)`, "
         "median of 5 calls after one warm-up, both optimisers in the same process on the same model.", "",
         "## multi_add wall time", "",
         "| N | device optimiser (ms) | side-by-side L-BFGS-B (ms) | ratio | device time inside (ms) | best acquisition per proposal: device | L-BFGS-B |",
         "|---|---|---|---|---|---|---|"]
    for r in rows:
        dv, lb = r["device"], r["fmin_l_bfgs_b"]
        L.append(f"| {r['N']} | {dv['ms']:.1f} | {lb['ms']:.1f} | {lb['ms'] / dv['ms']:.2f} | {dv['stats']['device_ms']:.1f} | "
                 f"{', '.join(f'{v:.3f}' for v in dv['acq'])} | {', '.join(f'{v:.3f}' for v in lb['acq'])} |")
    L += ["", "## One evaluation inside the kernel (two-pass form)", "",
          "40 uniform starts, one call; per evaluation = device_ms x nstart / sum(ncalls + ngrad); a value reads the lower "
          "triangle of V once (pass 1), a gradient once more (pass 2).", "",
          "| N | device_ms | evaluations | per evaluation (us) | bytes of V per pass (MB) | MB/us = TB/s per workgroup | status | iterations min / quartiles / max |",
          "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        st = ", ".join(f"{k} {v}" for k, v in r["status"].items() if v)
        L.append(f"| {r['N']} | {r['kernel_ms']:.2f} | {r['kernel_evals']} | {r['per_eval_us']:.1f} | {r['v_mb']:.2f} | "
                 f"{r['v_mb'] / r['per_eval_us']:.3f} | {st} | {' / '.join(str(v) for v in r['iters'])} |")
    L += ["", "## Gradient against the one-point predict", "",
          "max |G - ref| / max |ref| over the uniform points with sigma^2 - sigma_n^2 >= 0.01 C, "
          "ref = s (2 zeta mu_grad + std std_grad / (std^2 - sigma_n^2)):", ""]
    for r in rows:
        L.append(f"- N = {r['N']}: {r['grad_err']:.2e} over {r['grad_rows']} rows" if r["grad_err"] is not None else f"- N = {r['N']}: no row qualified")
    L += ["", "## Status of the optimiser path's ascents (summed over the 4 proposals of the last call)", ""]
    for r in rows:
        s = r["device"]["stats"]
        L.append(f"- N = {r['N']}: {s['device_status']}; {s['device_ncalls']} values, {s['device_ngrad']} gradients")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maximize_acq.md"))
    ap.add_argument("--sizes", default="256,1024,2048,4092")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child)
    rows = []
    for N in [int(v) for v in a.sizes.split(",")]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"N = {N}: no result within {CHILD_LIMIT_S} s; stopping", flush=True)
            break
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"N = {N}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            break
        rows.append(json.loads(res[-1][7:]))
        print(json.dumps(rows[-1]), flush=True)
    if rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table(rows))
        print(f"wrote {a.out}")
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())
