"""The mean under a batch of thetas on the device, timed: gpry_predict_thetas for B in {1, 32, 256} thetas and M in {1024,
65536} points on config1's model (N = 1024, d = 8, RBF) and on the bench's (N = 4096, d = 16, Matern-5/2): device time and
wall time of the call, its split into the factor chain and the point kernel from the two stage timers, the point kernel's
rate in kernel evaluations per second, and beside it the route there was before on the same context: one after another,
set_theta + factorize + predict, then putting the model back.  Thetas: the model's own as row 0, the others at
theta + 0.1 N(0, 1).  Prints the rows and writes a markdown table.

    python tools/time_predict_thetas.py [--md profiles/predict_thetas_times.md] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]


def sequential_route(dev, kid_flag, T, X):
    """set_theta + factorize + predict per theta, then the model put back: (means, wall ms)."""
    t0 = time.perf_counter()
    out = np.full((len(T), len(X)), np.nan)
    for b, th in enumerate(T):
        dev.set_theta(kid_flag, th)
        if dev.factorize() == 0:
            out[b] = dev.predict(X)
    dev.set_theta(kid_flag, T[0])
    assert dev.factorize() == 0
    return out, 1e3 * (time.perf_counter() - t0)


def rows_for(name, gpr, bounds, reps):
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
        base = dev.predict(X)
        for B in (1, 32, 256):
            T = Tall[:B]
            work, n = float(B) * M * N, reps
            dev.predict_thetas(T, X)
            ms, wall, chain, pts = [], [], [], []
            for _ in range(n):
                dev.timing_reset()
                t0 = time.perf_counter()
                out = dev.predict_thetas(T, X)
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(out["device_ms"])
                pts.append(dev.timing("predict_thetas_mean")[0])
                chain.append(dev.timing("predict_thetas")[0] - pts[-1])
            dev.set_option("timing", 0)
            assert np.array_equal(dev.predict(X), base), "the call disturbed the model"
            seq, seq_ms = sequential_route(dev, kid_flag, T, X)
            assert np.array_equal(dev.predict(X), base), "the model was not put back"
            ok = out["info"] == 0
            fin = ok[:, None] & np.isfinite(seq)                # (predict gates, the call does not: the points predict lets through)
            span = np.max(np.abs(seq[fin] - gpr._y_affine()[0])) if fin.any() else np.nan
            row = dict(model=name, N=N, B=B, M=M, reps=n, device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)),
                       chain_ms=float(np.median(chain)), points_ms=float(np.median(pts)), seq_ms=seq_ms, failed=int((~ok).sum()),
                       rate=work / (1e-3 * float(np.median(pts))), dev=float(np.max(np.abs(out["mean"][fin] - seq[fin])) / span) if fin.any() else float("nan"))
            print(f"{name}: B = {B}, M = {M}: call device {row['device_ms']:.2f} ms, wall {row['wall_ms']:.2f} ms (chain "
                  f"{row['chain_ms']:.2f}, points {row['points_ms']:.2f} = {row['rate']:.3g} kernel evaluations / s); one after another "
                  f"{seq_ms:.1f} ms = {seq_ms / row['wall_ms']:.2f} x the call; largest difference of the two {row['dev']:.1e} of the "
                  f"mean's range; {row['failed']} thetas not positive definite", flush=True)
            rows.append(row)
    return rows


def markdown(rows, device, reps):
    L = [f"Measured by `python tools/time_predict_thetas.py`, one {device}; medians of {reps} calls on a warm context; the "
         "sequential route once each, wall time, restoring the model included.", "",
         "| model | B | M | call: device ms | wall ms | chain ms | points ms | kernel evaluations / s | one after another, wall ms | "
         "sequential / call |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append(f"| {r['model']} | {r['B']} | {r['M']} | {r['device_ms']:.2f} | {r['wall_ms']:.2f} | {r['chain_ms']:.2f} | "
                 f"{r['points_ms']:.2f} | {r['rate']:.3g} | {r['seq_ms']:.1f} | {r['seq_ms'] / r['wall_ms']:.2f} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from time_maximize import models
    rows, device = [], None
    for name, gpr, bounds in reversed(list(models())):          # config1 first
        device = gpr.device.info()["arch"]
        rows += rows_for(name, gpr, bounds, args.reps)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(rows, device, args.reps))


if __name__ == "__main__":
    main()
