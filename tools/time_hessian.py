"""The Hessian of the surrogate's mean on the device, timed: gpry_hessian_mean at 1, 64 and 1024 points on config1's
model (N = 1024, d = 8, RBF) and on the bench's (N = 4096, d = 16, Matern-5/2), beside the only route there was before:
central differences over gpry_predict_grad_batch, 2 d gradient evaluations per point, batched as far as that call
allows (4096 points a call: the most favourable way to run it).  Then what covmat="laplace" does to the ascents:
iterations and device time of maximize_gp (64 starts) and of one profile_gp with the default H0 and with the Laplace
one, on the end-to-end models of the tests and on config1's.  Prints the rows and writes markdown tables.

    python tools/time_hessian.py [--md profiles/hessian_times.md] [--reps 5]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]


def fd_gradients(dev, Xfd):
    """The 2 d gradients per point of the central differences, in calls of gpry_predict_grad_batch's 4096 points at most."""
    for i in range(0, len(Xfd), 4096):
        dev.predict_grad_batch(Xfd[i:i + 4096], want_kinv=False)


def hessian_rows(name, gpr, bounds, reps):
    from gpry_amd.mc import _push_model
    _push_model(gpr, "hessian")
    dev, d = gpr.device, len(bounds)
    rng = np.random.default_rng(0)
    rows = []
    for n in (1, 64, 1024):
        X = rng.uniform(bounds[:, 0], bounds[:, 1], (n, d))
        h = 1e-5 * (bounds[:, 1] - bounds[:, 0])
        Xfd = np.ascontiguousarray((X[:, None, None, :] + np.array([1.0, -1.0])[None, None, :, None]
                                    * (np.eye(d) * h)[None, :, None, :]).reshape(-1, d))
        dev.hessian_mean(X)
        fd_gradients(dev, Xfd)
        ms, wall, fd = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = dev.hessian_mean(X)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(out["device_ms"])
            t0 = time.perf_counter()
            fd_gradients(dev, Xfd)
            fd.append(1e3 * (time.perf_counter() - t0))
        row = dict(model=name, n=n, device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)),
                   fd_wall_ms=float(np.median(fd)), fd_points=len(Xfd))
        print(f"{name}: {n} points: gpry_hessian_mean device {row['device_ms']:.3f} ms, wall {row['wall_ms']:.3f} ms; central "
              f"differences ({len(Xfd)} gradients through gpry_predict_grad_batch) wall {row['fd_wall_ms']:.3f} ms; ratio of "
              f"the walls {row['fd_wall_ms'] / row['wall_ms']:.1f}", flush=True)
        rows.append(row)
    return rows


def ascent_rows(name, gpr, bounds, reps):
    from gpry_amd.maximize import maximize_gp, profile_gp
    rows = []
    grid = np.linspace(bounds[0, 0] + 0.25 * (bounds[0, 1] - bounds[0, 0]), bounds[0, 1] - 0.25 * (bounds[0, 1] - bounds[0, 0]), 16)
    for cov in (None, "laplace"):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            maximize_gp(gpr, bounds=bounds, nstarts=8, covmat=cov)
            rs = [maximize_gp(gpr, bounds=bounds, nstarts=64, covmat=cov) for _ in range(reps)]
            ps = [profile_gp(gpr, 0, grid, bounds=bounds, nstarts=16, covmat=cov) for _ in range(reps)]
        r, p = rs[-1], ps[-1]
        row = dict(model=name, h0="Laplace" if cov else "default", fell_back=any("laplace" in str(w.message) for w in caught),
                   max_iters=int(r.iters.sum()), max_ncalls=int(r.ncalls.sum()), max_y=r.y,
                   max_device_ms=1e3 * float(np.median([q.device_s for q in rs])), prof_ncalls=int(p.ncalls),
                   prof_device_ms=1e3 * float(np.median([q.device_s for q in ps])), prof_y=float(np.max(p.y)))
        print(f"{name}, {row['h0']} H0{' (fell back)' if row['fell_back'] else ''}: maximize_gp 64 starts {row['max_iters']} "
              f"iterations, {row['max_ncalls']} evaluations, device {row['max_device_ms']:.2f} ms, best y {r.y:.9g}; profile_gp "
              f"16 x 16 starts {row['prof_ncalls']} evaluations, device {row['prof_device_ms']:.2f} ms", flush=True)
        rows.append(row)
    return rows


def markdown(hrows, arows, device, reps):
    L = [f"Measured by `python tools/time_hessian.py`, one {device}; medians of {reps} calls, warm context.", "",
         "| model | points | `gpry_hessian_mean` device ms | wall ms | central differences: gradients | wall ms | ratio of the walls |",
         "|---|---|---|---|---|---|---|"]
    for r in hrows:
        L.append(f"| {r['model']} | {r['n']} | {r['device_ms']:.3f} | {r['wall_ms']:.3f} | {r['fd_points']} | {r['fd_wall_ms']:.3f} | "
                 f"{r['fd_wall_ms'] / r['wall_ms']:.1f} |")
    L += ["", "| model | H0 | maximize_gp, 64 starts: iterations | evaluations | device ms | best y | profile_gp, 16 x 16 starts: "
          "evaluations | device ms |", "|---|---|---|---|---|---|---|---|"]
    for r in arows:
        L.append(f"| {r['model']} | {r['h0']}{' (fell back to the default)' if r['fell_back'] else ''} | {r['max_iters']} | "
                 f"{r['max_ncalls']} | {r['max_device_ms']:.2f} | {r['max_y']:.9g} | {r['prof_ncalls']} | {r['prof_device_ms']:.2f} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import maximize_numpy as mn
    import sampler_walk as sw
    from time_maximize import models
    hrows, arows, device = [], [], None
    for name, gpr, bounds in models():
        device = gpr.device.info()["arch"]
        hrows += hessian_rows(name, gpr, bounds, args.reps)
        if name.startswith("config1"):
            arows += ascent_rows(name, gpr, bounds, args.reps)
    for name, margs in mn.E2E_MODELS.items():
        m = sw.Model(**margs)
        arows += ascent_rows(f"tests' end-to-end model {name} (N = {m.N}, Matern-5/2)", m.gpr(), m.bounds, args.reps)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(hrows, arows, device, args.reps))


if __name__ == "__main__":
    main()
