"""Predictions without a group of training points on the device, timed: gpry_predict_without on config1's model (N = 1024,
d = 8, RBF) and on the bench's (N = 4096, d = 16, Matern-5/2) for one group of 16 with M = 1024 and M = 65536 points and for
"each" (N singletons) with M = 1024: device time and wall time of the call, its setup / points split (stage timers
"without_setup", "without_points", "without_panel", "without_contract"), the rate of the thin product beside the FP64 MFMA
rate this GPU measures (``microbench(2)``) and the rate of the panel build beside the sweep's panel kernel (stage
"cross_build" of a predict with std of the same points).  Beside it, in the same run on the same context:
``predict(return_std=True)`` of the same points (wall, and the sum of its kernels' stage timers), and the route there was
before -- the model reloaded without the rows, factorize, predict(return_std=True), the fitted model put back -- in wall
time; for "each" that route is timed for 4 groups and SCALED to N.  With --md, writes the markdown table of
profiles/predict_without.md.

    python tools/time_predict_without.py [--md times.md] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]

PREDICT_STAGES = ("cross_build", "sweep_mean", "sweep_gemm", "sweep_gemm_splitk", "sweep_finish", "gates")


def refactorising_route(dev, model, groups, X):
    """Per group: set_train without the rows, factorize, predict(return_std=True); then the model put back.  Wall ms."""
    X_, y_, al = model
    t0 = time.perf_counter()
    for g in groups:
        keep = np.setdiff1d(np.arange(len(y_)), g)
        dev.set_train(X_[keep], y_[keep], al[keep])
        assert dev.factorize() == 0
        dev.predict(X, return_std=True)
    dev.set_train(X_, y_, al)
    assert dev.factorize() == 0
    return 1e3 * (time.perf_counter() - t0)


def rows_for(name, gpr, bounds, reps, peak):
    from gpry_amd.mc import _push_model
    _push_model(gpr, "predict_without")
    dev, d = gpr.device, len(bounds)
    N = dev.N
    model = (np.asarray(gpr.X_train_, dtype=float), np.asarray(gpr.y_train_, dtype=float),
             np.array(np.broadcast_to(np.asarray(gpr.alpha, dtype=float), (N,))))
    rng = np.random.default_rng(0)
    rows = []
    for label, groups, M in (("one group of 16", [rng.choice(N, 16, replace=False)], 1024),
                             ("one group of 16", [rng.choice(N, 16, replace=False)], 65536),
                             ("each (N singletons)", [np.array([i]) for i in range(N)], 1024)):
        X = rng.uniform(bounds[:, 0], bounds[:, 1], (M, d))
        base = dev.predict(X, return_std=True)
        dev.predict_without(groups, X)
        ms, wall, st = [], [], {k: [] for k in ("without_setup", "without_points", "without_panel", "without_contract")}
        for _ in range(reps):
            dev.timing_reset()
            t0 = time.perf_counter()
            out = dev.predict_without(groups, X)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(out["device_ms"])
            for k in st:
                st[k].append(dev.timing(k)[0])
            dev.set_option("timing", 0)
        assert not out["info"].any()
        pwall, pstages, pcross = [], [], []
        for _ in range(reps):
            dev.timing_reset()
            t0 = time.perf_counter()
            after = dev.predict(X, return_std=True)
            pwall.append(1e3 * (time.perf_counter() - t0))
            pstages.append(sum(dev.timing(k)[0] for k in PREDICT_STAGES))
            pcross.append(dev.timing("cross_build")[0])
            dev.set_option("timing", 0)
        assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the call disturbed the model"
        timed = groups if len(groups) == 1 else groups[:4]
        route = refactorising_route(dev, model, timed, X) * len(groups) / len(timed)
        after = dev.predict(X, return_std=True)
        assert np.array_equal(after[0], base[0]) and np.array_equal(after[1], base[1]), "the model was not put back"
        med = {k: float(np.median(v)) for k, v in st.items()}
        rows_s = 16 * len(groups)                          # stacked rows, every group padded to 16
        con = med["without_contract"]
        useful = 2.0 * rows_s * N * M / (1e-3 * con) / 1e12
        tiles = 2.0 * max(128, -(-min(rows_s, 1024) // 128) * 128) * (-(-rows_s // 1024) if rows_s > 1024 else 1) * dev.N * M / (1e-3 * con) / 1e12
        row = dict(model=name, N=N, what=label, M=M, ngroups=len(groups), device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)),
                   predict_wall=float(np.median(pwall)), predict_stages=float(np.median(pstages)), route_ms=route,
                   scaled=len(timed) != len(groups), useful=useful, tiles=tiles, peak=peak,
                   panel_ns=1e6 * med["without_panel"] / (float(N) * M * (-(-rows_s // 1024))),
                   cross_ns=1e6 * float(np.median(pcross)) / (float(N) * M), **med)
        print(f"{name}: {label}, M = {M}: call device {row['device_ms']:.3f} ms, wall {row['wall_ms']:.3f} ms (setup {med['without_setup']:.3f}, "
              f"points {med['without_points']:.3f}: panel {med['without_panel']:.3f}, product {con:.3f}); predict(return_std=True) of the same "
              f"points: kernels {row['predict_stages']:.3f} ms, wall {row['predict_wall']:.3f} ms; refactorising route "
              f"{route:.1f} ms{' (4 groups timed, scaled to N)' if row['scaled'] else ''} = {route / row['wall_ms']:.2f} x the call; thin product "
              f"{useful:.2f} TFLOP/s on the groups' rows, {tiles:.2f} on the tiles the engine runs, of the measured {peak:.1f}; panel "
              f"{row['panel_ns']:.4f} ns per entry, the sweep's {row['cross_ns']:.4f}", flush=True)
        rows.append(row)
    return rows


def markdown(rows, device, reps, peak):
    L = [f"Measured by `python tools/time_predict_without.py`, one {device}; medians of {reps} calls on a warm context; the refactorising "
         f'route once each, wall time, putting the model back included; for "each" it is timed for 4 groups and SCALED to N.  FP64 MFMA rate '
         f"measured on the same GPU by `microbench(2)`: {peak:.1f} TFLOP/s.", "",
         "| model | groups | M | call: device ms | wall ms | setup ms | points ms | panel ms | product ms | predict(std): kernels ms | wall ms | "
         "refactorising route, wall ms | route / call | product TFLOP/s (rows / tiles) | panel ns per entry (call / sweep) |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append(f"| {r['model']} | {r['what']} | {r['M']} | {r['device_ms']:.3f} | {r['wall_ms']:.3f} | {r['without_setup']:.3f} | "
                 f"{r['without_points']:.3f} | {r['without_panel']:.3f} | {r['without_contract']:.3f} | {r['predict_stages']:.3f} | "
                 f"{r['predict_wall']:.3f} | {r['route_ms']:.1f}{' (scaled)' if r['scaled'] else ''} | {r['route_ms'] / r['wall_ms']:.2f} | "
                 f"{r['useful']:.2f} / {r['tiles']:.2f} | {r['panel_ns']:.4f} / {r['cross_ns']:.4f} |")
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
