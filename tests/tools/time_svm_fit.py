"""Times ``Device.svm_fit`` against scikit-learn's SVC (libsvm) on the same machine: profiles/svm_fit.md is its output.

    python tests/tools/time_svm_fit.py [--reps 5] [--out FILE]

Per (N, d) and eps: the labelled sets of tests/tools/svm_smo_numpy.py (half uniform in the unit cube, half around a
Gaussian mode, labelled by a threshold on the Gaussian log-density), C = 1e7, gamma = 1 / (d X.var()).  After one
warm-up of each side the two are timed in alternating pairs (device, libsvm, device, ...) and the medians reported:
device time (the call's events, copies included) and wall time of ``svm_fit``, its iterations and microseconds per
iteration, and libsvm's wall time and iterations.  One GPU, one process; nothing else should run on the card."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import svm_smo_numpy as sn  # noqa: E402

SHAPES = [(256, 4), (1024, 8), (2048, 8), (4096, 16), (8192, 16)]
EPS = (1e-3, 1e-10)


def main():
    from sklearn.svm import SVC
    from gpry_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _lib.Device(0)
    rows = []
    for N, d in SHAPES:
        X, finite = sn.labelled_set(N, d, seed=N + d)
        C, gamma = 1e7, 1.0 / (d * X.var())
        for eps in EPS:
            svc = SVC(C=C, kernel="rbf", gamma=gamma, tol=eps)
            res = dev.svm_fit(X, finite, C, gamma, eps=eps)             # warm-up of both sides
            svc.fit(X, finite)
            t_dev, t_wall, t_sk = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                res = dev.svm_fit(X, finite, C, gamma, eps=eps)
                t1 = time.perf_counter()
                svc.fit(X, finite)
                t2 = time.perf_counter()
                t_dev.append(res["device_ms"]); t_wall.append(1e3 * (t1 - t0)); t_sk.append(1e3 * (t2 - t1))
            row = dict(N=N, d=d, eps=eps, status=res["status"], n_iter=res["n_iter"], n_sv=int(np.count_nonzero(res["alpha"] > 0.0)),
                       device_ms=float(np.median(t_dev)), wall_ms=float(np.median(t_wall)),
                       us_per_iter=float(1e3 * np.median(t_dev) / max(res["n_iter"], 1)),
                       libsvm_ms=float(np.median(t_sk)), libsvm_iter=int(np.max(svc.n_iter_)), libsvm_n_sv=int(len(svc.support_)),
                       device_ms_min=float(np.min(t_dev)), device_ms_max=float(np.max(t_dev)),
                       libsvm_ms_min=float(np.min(t_sk)), libsvm_ms_max=float(np.max(t_sk)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n| N | d | eps | device ms (min-max) | wall ms | iterations | us / iteration | SVs | libsvm ms (min-max) | libsvm iterations | libsvm / device (wall) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['N']} | {r['d']} | {r['eps']:g} | {r['device_ms']:.2f} ({r['device_ms_min']:.2f}-{r['device_ms_max']:.2f}) | {r['wall_ms']:.2f} | "
              f"{r['n_iter']} | {r['us_per_iter']:.2f} | {r['n_sv']} | {r['libsvm_ms']:.2f} ({r['libsvm_ms_min']:.2f}-{r['libsvm_ms_max']:.2f}) | "
              f"{r['libsvm_iter']} | {r['libsvm_ms'] / r['wall_ms']:.2f} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
