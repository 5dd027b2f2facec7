"""The derivative of the predictive variance in theta on the device, timed: gpry_var_theta_grad for M in {1024, 65536}
points on config1's model (N = 1024, d = 8, RBF) and on the bench's (N = 4096, d = 16, Matern-5/2): device time and wall
time of the call, the setup (the d matrices dK / dlog l_a) and the per-panel stages apart (stage timers
"var_theta_grad_setup", "var_theta_grad_panel", "var_theta_grad_solve", "var_theta_grad_products",
"var_theta_grad_finish"), and the rate of the batched product dK_a Q -- 2 d N^2 flop per point -- as a fraction of the FP64
MFMA rate this GPU measures (``microbench(2)``, bench.py's probe).  Beside it the two routes there were before, both as
central differences with p = n_theta entries: 2 p times set_theta + factorize + predict(return_std=True) on the same
context, then putting the model back; and 2 p + 1 rows of predict_thetas(want_var=True) in one call.  Prints the rows and,
with --md, writes the markdown table that the section "Times" of profiles/var_theta_grad.md holds (written to a file of
its own and pasted there).

    python tools/time_var_theta_grad.py [--md times.md] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]

STAGES = ("var_theta_grad_setup", "var_theta_grad_panel", "var_theta_grad_solve", "var_theta_grad_products", "var_theta_grad_finish")
H = 1e-4


def sequential_route(dev, kid_flag, theta, X):
    """Central differences by refactorisation: 2 p times set_theta + factorize + predict(return_std=True), then the model put
    back: (G (M, p), wall ms)."""
    t0 = time.perf_counter()
    p = len(theta)
    G = np.full((len(X), p), np.nan)
    for j in range(p):
        v = []
        for sgn in (1.0, -1.0):
            th = theta.copy()
            th[j] += sgn * H
            dev.set_theta(kid_flag, th)
            v.append(dev.predict(X, return_std=True)[1] ** 2 if dev.factorize() == 0 else np.full(len(X), np.nan))
        G[:, j] = (v[0] - v[1]) / (2.0 * H)
    dev.set_theta(kid_flag, theta)
    assert dev.factorize() == 0
    return G, 1e3 * (time.perf_counter() - t0)


def thetas_route(dev, theta, X):
    """The same differences from one predict_thetas(want_var=True) call of 2 p + 1 rows: (G, wall ms, device ms)."""
    p = len(theta)
    rows = np.vstack([theta[None, :], theta[None, :] + H * np.eye(p), theta[None, :] - H * np.eye(p)])
    t0 = time.perf_counter()
    out = dev.predict_thetas(rows, X, want_var=True)
    wall = 1e3 * (time.perf_counter() - t0)
    return ((out["var"][1:p + 1] - out["var"][p + 1:]) / (2.0 * H)).T, wall, out["device_ms"]


def rows_for(name, gpr, bounds, reps, peak):
    from gpry_amd.mc import _push_model
    _push_model(gpr, "var_theta_grad")
    dev, d = gpr.device, len(bounds)
    kid_flag, theta = gpr._device_theta()
    theta = np.asarray(theta, dtype=float)
    N = dev.N
    rng = np.random.default_rng(0)
    rows = []
    for M in (1024, 65536):
        X = rng.uniform(bounds[:, 0], bounds[:, 1], (M, d))
        base = dev.predict(X, return_std=True)
        dev.var_theta_grad(X)
        ms, wall, st = [], [], {s: [] for s in STAGES}
        for _ in range(reps):
            dev.timing_reset()
            t0 = time.perf_counter()
            out = dev.var_theta_grad(X)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(out["device_ms"])
            for s in STAGES:
                st[s].append(dev.timing(s)[0])
        dev.set_option("timing", 0)
        after = dev.predict(X, return_std=True)
        assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the call disturbed the model"
        pt, pt_wall, pt_ms = thetas_route(dev, theta, X)
        seq, seq_ms = sequential_route(dev, kid_flag, theta, X)
        after = dev.predict(X, return_std=True)
        assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the model was not put back"
        med = {s: float(np.median(v)) for s, v in st.items()}
        prod = med["var_theta_grad_products"]
        tflops = 2.0 * d * M * float(N) * N / (1e-3 * prod) / 1e12
        big = np.max(np.abs(out["G"]))
        row = dict(model=name, N=N, d=d, M=M, reps=reps, device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)), **med,
                   tflops=tflops, frac=tflops / peak, seq_ms=seq_ms, pt_wall=pt_wall, pt_ms=pt_ms,
                   dev_seq=float(np.nanmax(np.abs(out["G"] - seq)) / big), dev_pt=float(np.nanmax(np.abs(out["G"] - pt)) / big))
        print(f"{name}: M = {M}: call device {row['device_ms']:.2f} ms, wall {row['wall_ms']:.2f} ms; setup "
              f"{med['var_theta_grad_setup']:.2f}, panel {med['var_theta_grad_panel']:.2f}, T and Q {med['var_theta_grad_solve']:.2f}, "
              f"products {prod:.2f} ms = {tflops:.2f} TFLOP/s = {row['frac']:.3f} of the measured {peak:.1f}, finish "
              f"{med['var_theta_grad_finish']:.2f}; {2 * len(theta)} refactorisations {seq_ms:.1f} ms = {seq_ms / row['wall_ms']:.2f} x the "
              f"call; {2 * len(theta) + 1} rows of predict_thetas {pt_wall:.1f} ms = {pt_wall / row['wall_ms']:.2f} x the call; largest "
              f"difference to their central differences {row['dev_seq']:.1e} / {row['dev_pt']:.1e} of the largest entry", flush=True)
        rows.append(row)
    return rows


def markdown(rows, device, reps, peak):
    L = [f"Measured by `python tools/time_var_theta_grad.py`, one {device}; medians of {reps} calls on a warm context; the two "
         f"comparators once each, wall time, restoring the model included.  FP64 MFMA rate measured on the same GPU by "
         f"`microbench(2)`: {peak:.1f} TFLOP/s; the batched product is counted as 2 d N^2 flop per point.", "",
         "| model | M | call: device ms | wall ms | setup ms | panel ms | T and Q ms | products ms | TFLOP/s | of the measured peak | "
         "finish ms | 2p refactorisations, wall ms | / call | 2p + 1 rows of predict_thetas, wall ms | / call |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append(f"| {r['model']} | {r['M']} | {r['device_ms']:.2f} | {r['wall_ms']:.2f} | {r['var_theta_grad_setup']:.2f} | "
                 f"{r['var_theta_grad_panel']:.2f} | {r['var_theta_grad_solve']:.2f} | {r['var_theta_grad_products']:.2f} | "
                 f"{r['tflops']:.2f} | {r['frac']:.3f} | {r['var_theta_grad_finish']:.2f} | {r['seq_ms']:.1f} | "
                 f"{r['seq_ms'] / r['wall_ms']:.2f} | {r['pt_wall']:.1f} | {r['pt_wall'] / r['wall_ms']:.2f} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from time_maximize import models
    rows, device, peak = [], None, None
    for name, gpr, bounds in reversed(list(models())):          # config1 first
        device = gpr.device.info()["arch"]
        if peak is None:
            gpr.device.microbench(2, 1)
            peak = gpr.device.microbench(2, 1)
        rows += rows_for(name, gpr, bounds, args.reps, peak)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(rows, device, args.reps, peak))


if __name__ == "__main__":
    main()
