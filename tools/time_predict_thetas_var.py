"""The predictive variance under a batch of thetas on the device, timed: gpry_predict_thetas_var for B in {1, 32, 256}
thetas and M in {1024, 65536} points on config1's model (N = 1024, d = 8, RBF) and on the bench's (N = 4096, d = 16,
Matern-5/2): device time and wall time of the call with ``want_var``, what it adds to the mean-only call, the variance
stage and inside it the matrix-pipe contraction (stage timers "predict_thetas_var", "predict_thetas_contract") with the
contraction's rate -- N^2 / 2 multiply-adds per theta and point -- as a fraction of the FP64 MFMA rate this GPU measures
(``microbench(2)``, bench.py's probe), and beside it the route there was before on the same context: one after another,
set_theta + factorize + predict(return_std=True), then putting the model back.  Thetas: the model's own as row 0, the
others at theta + 0.1 N(0, 1).  Prints the rows and, with --md, writes the markdown table that the section "Times" of
profiles/predict_thetas_var.md holds (written to a file of its own and pasted there).

    python tools/time_predict_thetas_var.py [--md times.md] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]


def sequential_route(dev, kid_flag, T, X):
    """set_theta + factorize + predict(return_std=True) per theta, then the model put back: (std^2, wall ms)."""
    t0 = time.perf_counter()
    out = np.full((len(T), len(X)), np.nan)
    for b, th in enumerate(T):
        dev.set_theta(kid_flag, th)
        if dev.factorize() == 0:
            out[b] = dev.predict(X, return_std=True)[1] ** 2
    dev.set_theta(kid_flag, T[0])
    assert dev.factorize() == 0
    return out, 1e3 * (time.perf_counter() - t0)


def rows_for(name, gpr, bounds, reps, peak):
    from gpry_amd.mc import _push_model
    _push_model(gpr, "predict_thetas")
    dev, d = gpr.device, len(bounds)
    kid_flag, theta = gpr._device_theta()
    theta = np.asarray(theta, dtype=float)
    N = dev.N
    rng = np.random.default_rng(0)
    Tall = np.vstack([theta[None, :], theta[None, :] + 0.1 * rng.standard_normal((255, len(theta)))])
    rows = []
    for M in (1024, 65536):
        X = rng.uniform(bounds[:, 0], bounds[:, 1], (M, d))
        base = dev.predict(X, return_std=True)
        for B in (1, 32, 256):
            T = Tall[:B]
            n = reps if float(B) * M * N * N < 1e14 else min(reps, 2)
            dev.predict_thetas(T, X, want_var=True)
            dev.predict_thetas(T, X)
            ms, wall, var_ms, con_ms, mean_only = [], [], [], [], []
            for _ in range(n):
                dev.timing_reset()
                t0 = time.perf_counter()
                out = dev.predict_thetas(T, X, want_var=True)
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(out["device_ms"])
                var_ms.append(dev.timing("predict_thetas_var")[0])
                con_ms.append(dev.timing("predict_thetas_contract")[0])
                dev.set_option("timing", 0)
                mean_only.append(dev.predict_thetas(T, X)["device_ms"])
            dev.set_option("timing", 0)
            after = dev.predict(X, return_std=True)
            assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the call disturbed the model"
            seq, seq_ms = sequential_route(dev, kid_flag, T, X)
            after = dev.predict(X, return_std=True)
            assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the model was not put back"
            ok = out["info"] == 0
            fin = ok[:, None] & np.isfinite(seq)
            prior = np.max(out["var"][ok]) if ok.any() else np.nan
            con = float(np.median(con_ms))
            tflops = float(B) * M * float(N) * N / (1e-3 * con) / 1e12          # N^2 / 2 multiply-adds = N^2 flop
            row = dict(model=name, N=N, B=B, M=M, reps=n, device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)),
                       mean_only_ms=float(np.median(mean_only)), var_ms=float(np.median(var_ms)), con_ms=con, tflops=tflops,
                       frac=tflops / peak, seq_ms=seq_ms, failed=int((~ok).sum()),
                       dev=float(np.max(np.abs(out["var"][fin] - seq[fin])) / prior) if fin.any() else float("nan"))
            print(f"{name}: B = {B}, M = {M}: call device {row['device_ms']:.2f} ms, wall {row['wall_ms']:.2f} ms; mean-only call "
                  f"{row['mean_only_ms']:.2f} ms, added {row['device_ms'] - row['mean_only_ms']:.2f}; variance stage {row['var_ms']:.2f} ms, "
                  f"contraction {con:.2f} ms = {tflops:.2f} TFLOP/s = {row['frac']:.3f} of the measured {peak:.1f}; one after another "
                  f"{seq_ms:.1f} ms = {seq_ms / row['wall_ms']:.2f} x the call; largest difference of the two {row['dev']:.1e} of the "
                  f"largest variance; {row['failed']} thetas not positive definite", flush=True)
            rows.append(row)
    return rows


def markdown(rows, device, reps, peak):
    L = [f"Measured by `python tools/time_predict_thetas_var.py`, one {device}; medians of {reps} calls on a warm context (2 where "
         f"B M N^2 >= 1e14); the sequential route once each, wall time, restoring the model included.  FP64 MFMA rate measured on the "
         f"same GPU by `microbench(2)`: {peak:.1f} TFLOP/s; the contraction is counted as N^2 flop per theta and point.", "",
         "| model | B | M | call: device ms | wall ms | mean-only call ms | added ms | variance stage ms | contraction ms | TFLOP/s | of the "
         "measured peak | one after another, wall ms | sequential / call |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append(f"| {r['model']} | {r['B']} | {r['M']} | {r['device_ms']:.2f} | {r['wall_ms']:.2f} | {r['mean_only_ms']:.2f} | "
                 f"{r['device_ms'] - r['mean_only_ms']:.2f} | {r['var_ms']:.2f} | {r['con_ms']:.2f} | {r['tflops']:.2f} | {r['frac']:.3f} | "
                 f"{r['seq_ms']:.1f} | {r['seq_ms'] / r['wall_ms']:.2f} |")
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
