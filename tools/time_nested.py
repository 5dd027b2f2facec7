"""Nested sampling of the surrogate on the device at the reference's defaults, on the bench's fitted model (BASELINE
configs[2]: N = 4096, d = 16): wall and device time per run, evaluations and evaluations per second, for several
batch sizes (chains per generation), against the per-call time of the one-point gpr.predict measured in the same
process; then one full NORA.multi_add with sampler="nested".

    python tools/time_nested.py [--runs 3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import bench
    from gpry_amd.gp_acquisition import NORA
    from gpry_amd.nested import run_nested
    N, d, M = 4096, 16, 1000
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    out = {"N": gpr.n, "d": d, "device": gpr.device.info()["arch"]}
    # one-point predict, as a point-by-point sampler calls it
    for x in Xc[:50]:
        gpr.predict(x[None, :], validate=False)
    t0 = time.perf_counter()
    for x in Xc[:1000]:
        gpr.predict(x[None, :], validate=False)
    t_pt = (time.perf_counter() - t0) / 1000
    out["predict_one_point_us"] = t_pt * 1e6
    print(f"one-point gpr.predict: {t_pt * 1e6:.2f} us per call = {1 / t_pt:.3g} evaluations/s")
    acq = NORA(bounds, sampler="nested", verbose=0, devices=[0])
    prec = acq.update_NS_precision(gpr)
    out["settings"] = prec
    print(f"settings: {prec}")
    assert gpr._push_gates()
    nlive = prec["nlive"]
    out["runs"] = {}
    for k in (nlive // 8, nlive // 4, nlive // 2):
        rows = []
        for seed in range(args.runs + 1):
            r = run_nested(gpr.device, bounds, 100 + seed, nlive, prec["num_repeats"],
                           precision_criterion=prec["precision_criterion"], nprior=prec["nprior"],
                           max_ncalls=prec["max_ncalls"], batch=k, minus_inf_value=gpr.minus_inf_value)
            if seed == 0:
                continue          # (first run loads the code objects)
            rows.append(dict(wall_s=r.wall_s, device_s=r.device_s, ncalls=r.ncalls, generations=r.ngen,
                             evals_per_s=r.ncalls / r.device_s, logZ=r.logZ, logZ_err=r.logZ_err, rows=len(r.y)))
        med = {key: float(np.median([row[key] for row in rows])) for key in rows[0]}
        out["runs"][str(k)] = {"median": med, "all": rows}
        print(f"batch {k:4d}: wall {med['wall_s']:.3f} s, device {med['device_s']:.3f} s, {med['ncalls']:.3g} evaluations, "
              f"{med['generations']:.0f} generations, {med['evals_per_s']:.3g} evaluations/s "
              f"({med['evals_per_s'] * t_pt:.0f}x the one-point rate), logZ {med['logZ']:.3f} +- {med['logZ_err']:.3f}")
    # one full acquisition step
    acq.multi_add(gpr, n_points=1, rng=np.random.default_rng(0))        # warm-up
    t0 = time.perf_counter()
    acq.multi_add(gpr, n_points=4, rng=np.random.default_rng(1))
    t_ma = time.perf_counter() - t0
    out["multi_add_s"] = t_ma
    out["multi_add_sampler_info"] = acq.stats["sampler_info"]
    print(f"multi_add(n_points=4, sampler='nested'): {t_ma:.3f} s; sampler {acq.stats['sampler_info']}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1, default=float)


if __name__ == "__main__":
    main()
