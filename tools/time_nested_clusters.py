"""Clustering in the device nested sampler, measured (profiles/nested_clusters.md).

    python tools/time_nested_clusters.py knn [--json out.json]     # gpry_ns_knn at n in {400, 800, 1600, 6400}, d in {16, 32}
    python tools/time_nested_clusters.py runs [--runs 3] [--json out.json]

``knn``: device time of gpry_ns_knn (k = 10, the default cluster_k_max) per call; run it under
``rocprofv3 --kernel-trace --stats`` for the kernels' own times.  ``runs``: full run_nested runs with clustering off and on,
on the bench's fitted model (N = 4096, d = 16, unimodal: the overhead) and on a fitted bimodal surrogate (d = 4: the
benefit), at NORA's settings for the model; wall and device time, evaluations, generations, cluster counts, logZ, the
host time of knn_clusters and of the whitening matrices per generation, and (bimodal) each mode's mass against a
quadrature of gpr.predict.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _model(d, N=256):
    import bench
    bounds, X, y, Xc, _ = bench.synthetic(N - d, d, 16)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    return gpr


def knn(args):
    out = {"k": 10, "rows": []}
    for d in (16, 32):
        dev = _model(d).device
        rng = np.random.default_rng(d)
        lo, hi = np.zeros(d), np.ones(d)
        for n in (400, 800, 1600, 6400):
            X = rng.uniform(size=(n, d))
            dev.ns_knn(lo, hi, X, 10)                 # (loads the code object)
            ms = [dev.ns_knn(lo, hi, X, 10)[1] for _ in range(args.runs)]
            row = dict(n=n, d=d, call_ms_median=float(np.median(ms)), call_ms_min=float(np.min(ms)))
            out["rows"].append(row)
            print(f"ns_knn n={n:5d} d={d:2d} k=10: {row['call_ms_median']:.3f} ms per call (median of {args.runs})")
    return out


def _timed(nested):
    """Wraps nested.knn_clusters / nested.whitening with clocks; returns the totals dict."""
    tot = {"knn_clusters_s": 0.0, "whitening_s": 0.0}
    real_kc, real_w = nested.knn_clusters, nested.whitening

    def kc(*a, **k):
        t0 = time.perf_counter()
        r = real_kc(*a, **k)
        tot["knn_clusters_s"] += time.perf_counter() - t0
        return r

    def wh(*a, **k):
        t0 = time.perf_counter()
        r = real_w(*a, **k)
        tot["whitening_s"] += time.perf_counter() - t0
        return r

    nested.knn_clusters, nested.whitening = kc, wh
    return tot, (real_kc, real_w)


def _runs(name, gpr, bounds, prec, nruns, frac_of=None):
    from gpry_amd import nested
    res = {}
    for clustering in (False, True):
        rows = []
        for seed in range(nruns + 1):
            tot, real = _timed(nested)
            try:
                r = nested.run_nested(gpr.device, bounds, 100 + seed, prec["nlive"], prec["num_repeats"],
                                      precision_criterion=prec["precision_criterion"], nprior=prec["nprior"],
                                      max_ncalls=prec["max_ncalls"], minus_inf_value=gpr.minus_inf_value,
                                      clustering=clustering)
            finally:
                nested.knn_clusters, nested.whitening = real
            if seed == 0:
                continue          # (first run loads the code objects)
            row = dict(wall_s=r.wall_s, device_s=r.device_s, ncalls=r.ncalls, generations=r.ngen, logZ=r.logZ,
                       logZ_err=r.logZ_err, rows=len(r.y),
                       host_knn_clusters_ms_per_gen=1e3 * tot["knn_clusters_s"] / max(r.ngen, 1),
                       host_whitening_ms_per_gen=1e3 * tot["whitening_s"] / max(r.ngen, 1))
            if clustering:
                row["clusters_hist"] = np.bincount(r.n_clusters).tolist()
                row["clusters_max"] = int(r.n_clusters.max())
            if frac_of is not None:
                row["mass_x0_negative"] = float(np.sum(r.w[r.X[:, 0] < 0]))
            rows.append(row)
        med = {k: float(np.median([row[k] for row in rows])) for k in rows[0] if not isinstance(rows[0][k], list)}
        res["on" if clustering else "off"] = {"median": med, "all": rows}
        print(f"{name} clustering {'on ' if clustering else 'off'}: wall {med['wall_s']:.3f} s, device {med['device_s']:.3f} s, "
              f"{med['ncalls']:.4g} evaluations, {med['generations']:.0f} generations, logZ {med['logZ']:.3f} +- "
              f"{med['logZ_err']:.3f}, host knn_clusters {med['host_knn_clusters_ms_per_gen']:.3f} ms/gen, whitening "
              f"{med['host_whitening_ms_per_gen']:.3f} ms/gen"
              + (f", clusters {[r['clusters_hist'] for r in rows]}" if clustering else "")
              + (f", mass(x0<0) {[round(r['mass_x0_negative'], 3) for r in rows]} (quadrature {frac_of:.3f})"
                 if frac_of is not None else ""))
    return res


def runs(args):
    import bench
    from gpry_amd.gp_acquisition import NORA
    from test_nested_cluster_gpu import _fitted_bimodal
    from test_nested_gpu import _quadrature
    out = {}
    # the bench's fitted model (unimodal)
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
    # a fitted bimodal surrogate
    d = 4
    gpr, bounds = _fitted_bimodal(d, 500)
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    n = 40
    axes = [bounds[k, 0] + (np.arange(n) + 0.5) * (bounds[k, 1] - bounds[k, 0]) / n for k in range(d)]
    G = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    yg = gpr.predict(G)
    pg = np.exp(yg - yg.max())
    frac_q = float(np.sum(pg[G[:, 0] < 0]) / np.sum(pg))
    logZq = float(_quadrature(gpr, bounds, n)[0])
    gpr._push_gates()
    prec = NORA(bounds, sampler="nested", verbose=0, devices=[0]).update_NS_precision(gpr)
    out["bimodal"] = {"N": gpr.n, "d": d, "settings": prec, "quadrature_logZ": logZq, "quadrature_mass_x0_negative": frac_q,
                      **_runs("bimodal N=500 d=4", gpr, bounds, prec, args.runs, frac_of=frac_q)}
    print(f"bimodal quadrature: logZ {logZq:.3f}, mass(x0<0) {frac_q:.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["knn", "runs"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = knn(args) if args.what == "knn" else runs(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1, default=float)


if __name__ == "__main__":
    main()
