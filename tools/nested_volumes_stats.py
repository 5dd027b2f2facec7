"""Per-cluster prior volumes in the nested sampler, measured (profiles/nested_volumes.md).

    python tools/nested_volumes_stats.py cpu [--seeds 24] [--json out.json]   # numpy stand-in, analytic mixtures
    python tools/nested_volumes_stats.py gpu [--seeds 16] [--json out.json]   # fitted bimodal surrogate, on the device
    python tools/nested_volumes_stats.py runs [--runs 3] [--json out.json]    # wall / device / host time, off vs on

``cpu``: the small mode's mass, sum(w) over x_0 < 0, of the analytic two-Gaussian mixture of
tests/test_nested_volumes_cpu.py (2 dimensions, modes at x_0 = -2 and +2, sigma 0.3, box [-5, 5]^2; num_repeats 10,
nprior 10 nlive) with clustering on, per-cluster volumes off and on, over the same seeds: its RMS error against the
truth, its range, and how often the mode is lost (mass below a third of the truth).  ``gpu``: the same statistics on the
fitted bimodal surrogate of tests/test_nested_cluster_gpu.py (d = 4) against a 40^4-cell quadrature of gpr.predict.
``runs``: the bench's fitted model (N = 4096, d = 16) and the bimodal surrogate at NORA's settings, clustering on with
volumes off and on: wall and device time, the host time per generation outside the device calls, and the wall time of
the neighbour-table calls per generation.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]


def stats(masses, truth):
    m = np.asarray(masses)
    return dict(truth=truth, rms=float(np.sqrt(np.mean((m - truth) ** 2))), min=float(m.min()), max=float(m.max()),
                lost=int(np.sum(m < truth / 3)), masses=[float(v) for v in m])


def cpu(args):
    import ns_volumes
    from gpry_amd.nested import run_nested
    from test_nested_volumes_cpu import _small_mode_mixture
    out = []
    for f, nlive in ((0.15, 100), (0.15, 50), (0.05, 100), (0.05, 50), (0.05, 25)):
        loglike, bounds, _ = _small_mode_mixture(f)
        row = dict(weight=f, nlive=nlive, binomial=float(np.sqrt(f * (1 - f) / nlive)))
        for vol in (False, True):
            masses = []
            for seed in range(args.seeds):
                r = run_nested(ns_volumes.VolumesNumpyDevice(loglike), bounds, 1000 + seed, nlive=nlive, num_repeats=10,
                               nprior=10 * nlive, clustering=True, cluster_volumes=vol)
                masses.append(np.sum(r.w[r.X[:, 0] < 0]))
            row["on" if vol else "off"] = stats(masses, f)
        out.append(row)
        print(f"f={f} nlive={nlive} (binomial {row['binomial']:.3f}): "
              + ", ".join(f"volumes {k}: rms {row[k]['rms']:.3f} range {row[k]['min']:.3f} .. {row[k]['max']:.3f} "
                          f"lost {row[k]['lost']}/{args.seeds}" for k in ("off", "on")), flush=True)
    return out


def _bimodal():
    from test_nested_cluster_gpu import _fitted_bimodal
    from test_nested_gpu import _quadrature
    d, n = 4, 40
    gpr, bounds = _fitted_bimodal(d, 500)
    gpr._ensure_factor()
    gpr._push_affine()
    axes = [bounds[k, 0] + (np.arange(n) + 0.5) * (bounds[k, 1] - bounds[k, 0]) / n for k in range(d)]
    G = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    yg = gpr.predict(G)
    pg = np.exp(yg - yg.max())
    frac_q = float(np.sum(pg[G[:, 0] < 0]) / np.sum(pg))
    logZq = float(_quadrature(gpr, bounds, n)[0])
    assert gpr._push_gates()
    return gpr, bounds, logZq, frac_q


def gpu(args):
    from gpry_amd.nested import run_nested
    gpr, bounds, logZq, frac_q = _bimodal()
    out = dict(quadrature_logZ=logZq, quadrature_mass=frac_q, rows=[])
    for nlive in (25, 50, 100, 200):
        row = dict(nlive=nlive)
        for vol in (False, True):
            masses, dz = [], []
            for seed in range(args.seeds):
                r = run_nested(gpr.device, bounds, 1000 + seed, nlive, 20, nprior=10 * nlive,
                               minus_inf_value=gpr.minus_inf_value, clustering=True, cluster_volumes=vol)
                masses.append(np.sum(r.w[r.X[:, 0] < 0]))
                dz.append((r.logZ - logZq) / r.logZ_err)
            row["on" if vol else "off"] = {**stats(masses, frac_q), "logZ_pull_max": float(np.max(np.abs(dz)))}
        out["rows"].append(row)
        print(f"bimodal nlive={nlive} (quadrature mass {frac_q:.3f}): "
              + ", ".join(f"volumes {k}: rms {row[k]['rms']:.3f} range {row[k]['min']:.3f} .. {row[k]['max']:.3f} "
                          f"lost {row[k]['lost']}/{args.seeds} max |dlogZ|/err {row[k]['logZ_pull_max']:.2f}"
                          for k in ("off", "on")), flush=True)
    return out


class _Timed:
    """A device whose ns_knn calls are clocked."""

    def __init__(self, dev):
        self.dev, self.knn_s, self.knn_calls = dev, 0.0, 0

    def __getattr__(self, name):
        return getattr(self.dev, name)

    def ns_knn(self, *a):
        t0 = time.perf_counter()
        r = self.dev.ns_knn(*a)
        self.knn_s += time.perf_counter() - t0
        self.knn_calls += 1
        return r


def _runs(name, gpr, bounds, prec, nruns):
    from gpry_amd.nested import run_nested
    res = {}
    for vol in (False, True):
        rows = []
        for seed in range(nruns + 1):
            dev = _Timed(gpr.device)
            r = run_nested(dev, bounds, 100 + seed, prec["nlive"], prec["num_repeats"],
                           precision_criterion=prec["precision_criterion"], nprior=prec["nprior"],
                           max_ncalls=prec["max_ncalls"], minus_inf_value=gpr.minus_inf_value, clustering=True,
                           cluster_volumes=vol)
            if seed == 0:
                continue          # (first run loads the code objects)
            rows.append(dict(wall_s=r.wall_s, device_s=r.device_s, ncalls=r.ncalls, generations=r.ngen, logZ=r.logZ,
                             host_ms_per_gen=1e3 * (r.wall_s - r.device_s) / max(r.ngen, 1),
                             knn_wall_ms_per_gen=1e3 * dev.knn_s / max(r.ngen, 1),
                             knn_calls_per_gen=dev.knn_calls / max(r.ngen, 1), clusters_max=int(r.n_clusters.max())))
        med = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
        res["on" if vol else "off"] = {"median": med, "all": rows}
        print(f"{name} volumes {'on ' if vol else 'off'}: wall {med['wall_s'] * 1e3:.1f} ms, device "
              f"{med['device_s'] * 1e3:.1f} ms, {med['ncalls']:.4g} evaluations, {med['generations']:.0f} generations, "
              f"host {med['host_ms_per_gen']:.3f} ms/gen, knn calls {med['knn_calls_per_gen']:.2f}/gen taking "
              f"{med['knn_wall_ms_per_gen']:.3f} ms/gen, clusters max {med['clusters_max']:.0f}", flush=True)
    return res


def runs(args):
    import bench
    from gpry_amd.gp_acquisition import NORA
    out = {}
    N, d = 4096, 16
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, 1000)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    prec = NORA(bounds, sampler="nested", verbose=0, devices=[0]).update_NS_precision(gpr)
    out["bench_model"] = {"N": gpr.n, "d": d, "settings": prec,
                          **_runs("bench model N=4096 d=16", gpr, bounds, prec, args.runs)}
    gpr, bounds, logZq, frac_q = _bimodal()
    prec = NORA(bounds, sampler="nested", verbose=0, devices=[0]).update_NS_precision(gpr)
    out["bimodal"] = {"N": gpr.n, "d": 4, "settings": prec, **_runs("bimodal N=500 d=4", gpr, bounds, prec, args.runs)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cpu", "gpu", "runs"])
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = {"cpu": cpu, "gpu": gpu, "runs": runs}[args.what](args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1, default=float)


if __name__ == "__main__":
    main()
