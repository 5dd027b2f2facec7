"""Times the batched leave-one-out objective and the side-by-side ``"loo"`` fit: profiles/loo_fit_batch.md is its output.

    python tests/tools/time_loo_batch.py [--reps 11] [--root TREE] [--skip-fit] [--out FILE]

(a) 32 thetas with gradient: one ``loo_objective_batch`` against 32 ``loo_objective`` calls, at (1024, 8) RBF and
    (4096, 16) Matern-5/2 -- wall time of the calls (each ends in a stream synchronise; the two forms alternate repeat by
    repeat) and, in a run of its own with the library's stage timers on, device time: the ``loo_batch`` timer around the
    chunk against the sum of the per-stage timers of the 32 single chains, and the batch's own split by stage.
(b) the default-restart (10 + 2 d) ``"loo"`` fit at N = 400 / 1024 / 2048, d = 8: side by side against sequential, same
    seed, same data; the two must end at the same theta.
``--root`` points at another checkout of the project (with its library built) to measure that one instead: on a tree
without ``loo_objective_batch`` only the sequential forms are timed.  Medians over ``--reps`` repeats after two warm-up
repeats, with the smallest and the largest.  One GPU, one process; nothing else should run on the card."""
import argparse
import json
import os
import sys
import time

import numpy as np

STAGES = ("kernel_build", "potrf", "trtri", "solve_alpha", "loo_q", "lauum", "loo_mirror", "loo_gram", "loo_traces")


def model(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.standard_normal(N)
    theta = np.log(np.append(2.0, rng.uniform(0.2, 0.6, d)))
    thetas = theta + rng.uniform(-0.2, 0.2, (32, d + 1))
    return X, (y - y.mean()) / y.std(), np.full(N, 1e-4), theta, thetas


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def evaluations(_lib, N, d, kid, reps):
    X, y_, a, theta, T = model(N, d, N + d)
    dev = _lib.Device(0)
    try:
        dev.set_train(X, y_, a)
        dev.set_theta(kid, theta)
        forms = {"32 single calls": lambda: [dev.loo_objective(T[j], True) for j in range(len(T))]}
        if hasattr(dev, "loo_objective_batch"):
            forms["one batched call"] = lambda: dev.loo_objective_batch(T, True)
        wall = {k: [] for k in forms}
        for rep in range(reps + 2):
            for k, f in forms.items():
                t0 = time.perf_counter()
                out = f()
                if rep >= 2:
                    wall[k].append(1e3 * (time.perf_counter() - t0))
        row = dict(N=N, d=d, kernel=kid, thetas=len(T), wall_ms={k: stats(v) for k, v in wall.items()})
        if "one batched call" in forms:
            one = forms["32 single calls"]()
            val, grad, info = forms["one batched call"]()
            row["same_bits"] = bool(all(val[j] == one[j][0] and np.array_equal(grad[j], one[j][1]) for j in range(len(T))))
        # device time, timers on: their events cost a little per stage, so this run is separate from the wall times
        device = {}
        for k, f in forms.items():
            per = []
            for rep in range(reps + 2):
                dev.timing_reset()
                f()
                if k == "one batched call":
                    t = dev.timing("loo_batch")[0]
                    stages = {s: dev.timing(s)[0] for s in STAGES}
                else:
                    t = sum(dev.timing(s)[0] for s in STAGES)
                if rep >= 2:
                    per.append(t)
            device[k] = stats(per)
            if k == "one batched call":
                row["batch_stage_ms"] = {s: round(v, 4) for s, v in stages.items()}
            else:
                row["single_stage_ms_sum32"] = {s: round(dev.timing(s)[0], 4) for s in STAGES}
        row["device_ms"] = device
        del out
        return row
    finally:
        dev.close()


def fits(N, d, reps):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import ConstantKernel as C, Matern, WhiteKernel
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    rng = np.random.default_rng(N)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(N)
    bounds = np.array([[0.0, 1.0]] * d)

    def fit(side_by_side):
        kernel = C(1.0, [1e-3, 1e4]) * Matern(np.ones(d), [1e-3, 10.], nu=2.5) + WhiteKernel(1e-2, [1e-6, 1e1])
        g = GaussianProcessRegressor(kernel=kernel, bounds=bounds, n_restarts_optimizer=10 + 2 * d, noise_level=1e-2,
                                     preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(),
                                     account_for_inf=None, random_state=5)
        g.fit_devices = [0]
        g.append_to_data(X, y, fit_gpr=False)
        kw = {"side_by_side": True} if side_by_side else {}
        n0 = g.n_eval_loglike
        t0 = time.perf_counter()
        g.fit_gpr_hyperparameters(objective="loo", **kw)
        return 1e3 * (time.perf_counter() - t0), g, g.n_eval_loglike - n0

    import inspect
    forms = {"sequential": False}
    if "side_by_side" in inspect.signature(GaussianProcessRegressor.fit_gpr_hyperparameters).parameters:
        forms["side by side"] = True
    ms, last, evals = {k: [] for k in forms}, {}, {}
    for rep in range(reps + 2):
        for k, sbs in forms.items():
            dt, g, n = fit(sbs)
            if rep >= 2:
                ms[k].append(dt)
            last[k], evals[k] = g, n
    row = dict(N=N, d=d, restarts=10 + 2 * d, fit_ms={k: stats(v) for k, v in ms.items()}, evaluations=evals,
               loo_value={k: float(g.loo_value_) for k, g in last.items()},
               fit_stats={k: {s: v for s, v in g.fit_stats.items() if s in ("side_by_side", "why", "contexts", "schedule")}
                          for k, g in last.items()})
    if len(last) == 2:
        row["same_theta"] = bool(np.array_equal(last["sequential"].kernel_.theta, last["side by side"].kernel_.theta))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from gpry_amd import _lib
    rows = []
    for N, d, kid in ((1024, 8, 0), (4096, 16, 3)):
        rows.append(dict(what="evaluations", **evaluations(_lib, N, d, kid, args.reps)))
        print(json.dumps(rows[-1]), flush=True)
    if not args.skip_fit:
        for N in (400, 1024, 2048):
            rows.append(dict(what="fit", **fits(N, 8, args.reps)))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(root=os.path.abspath(args.root), reps=args.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
