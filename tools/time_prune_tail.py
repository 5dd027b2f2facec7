"""The tail of the pruned NORA sweep behind stage A, at BASELINE configs[2] (N = 4096, d = 16, M = 1e6): median over repeated
`multi_add` calls on a resident pool of the HIP-event stage timers "sweep_mean", "sweep_prune_select", "sweep_compact",
"sweep_prune_gemm", "topk" and of the wall time, with each of the options "sweep_small_map", "select_fused" and
"prune_one_select" on (the default) and off, on the bench's fitted model and on theta = log[4, 0.3...].

    python tools/time_prune_tail.py [--reps 9] [--model 0|1] [--json out.json]

Every variant proposes the same points (checked).  The figures per variant are per multi_add call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STAGES = ("sweep_mean", "sweep_prune_select", "sweep_compact", "sweep_prune_gemm", "topk")
OPTIONS = ("sweep_small_map", "select_fused", "prune_one_select")


def models(N, d, M):
    import bench
    from oracle import gpry_oracle as orc
    from test_host_mirror_gpu import make_gpr
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    yield "bench fitted model", gpr, bounds, Xc
    bounds, X, y, Xc = orc.synthetic_problem(N, d, M)
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.log(np.array([4.0] + [0.3] * d)))
    gpr.append_to_data(X, y, fit_gpr=False)
    yield "theta = log[4, 0.3...]", gpr, bounds, Xc


def run(gpr, bounds, Xc, reps):
    from gpry_amd.gp_acquisition import NORA
    dev = gpr.device
    acq = NORA(bounds, sampler="uniform", mc_every=1, verbose=0, devices=[0])
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)    # (one array: resident)
    variants = [("all on", {})] + [(f"{o} = 0", {o: 0}) for o in OPTIONS] + [("all off", {o: 0 for o in OPTIONS})]
    res, ref = {}, None
    dev.set_option("timing", 1)
    try:
        for name, off in variants:
            for o in OPTIONS:
                dev.set_option(o, off.get(o, 1))
            rows = []
            for r in range(reps + 1):
                dev.timing_reset()
                t0 = time.perf_counter()
                Xp, _, ap = acq.multi_add(gpr, n_points=gpr.d, rng=np.random.default_rng(2))
                wall = (time.perf_counter() - t0) * 1e3
                if ref is None:
                    ref = (Xp.copy(), ap.copy())
                assert np.array_equal(Xp, ref[0]) and np.array_equal(ap, ref[1]), name
                if r:                                       # (the first call is a warm-up)
                    rows.append([dev.timing(s)[0] for s in STAGES] + [wall])
            rows = np.array(rows)
            med = np.median(rows, axis=0)
            res[name] = {k: float(v) for k, v in zip(STAGES + ("wall",), med)}
            res[name]["wall_min"] = float(rows[:, -1].min())
            res[name]["wall_max"] = float(rows[:, -1].max())
            res[name]["launches"] = {s: dev.timing(s)[1] for s in STAGES}
            res[name]["prune_info"] = {k: v for k, v in dev.sweep_prune_info().items() if k != "stage_ms"}
    finally:
        for o in OPTIONS:
            dev.set_option(o, 1)
        dev.set_option("timing", 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--model", type=int, default=None, help="0: the bench's fitted model, 1: theta = log[4, 0.3...]")
    a = ap.parse_args()
    out = {}
    for i, (label, gpr, bounds, Xc) in enumerate(models(4096, 16, 1_000_000)):
        if a.model is not None and i != a.model:
            continue
        out[label] = run(gpr, bounds, Xc, a.reps)
        for name, r in out[label].items():
            print(f"{label:24s} {name:22s} " + " ".join(f"{s} {r[s]:7.3f}" for s in STAGES) +
                  f"  wall {r['wall']:7.2f} ms [{r['wall_min']:.2f}, {r['wall_max']:.2f}]  "
                  f"contracted {r['prune_info']['contracted']} rounds {r['prune_info']['rounds']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
