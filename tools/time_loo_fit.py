"""The measurements of profiles/loo_fit.md: one ``gpry_loo_objective`` with gradient beside one ``gpry_lml`` with gradient
on the same model (wall time of the call, which ends in a stream synchronise; the two alternate call by call), the
split by stage through the library's stage timers (a run of their own: the timers add two events per stage), one full
``objective="loo"`` fit beside the sequential LML fit of the same model at N = 1024, and the leave-one-out calibration
(``validate_gp``) after an LML fit and after a leave-one-out fit of an RBF model to Matern-1/2-rough data.  Sizes: config1
(N = 1024, d = 8) and N = 4096, d = 16, the models of tools/time_loo.py."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np  # noqa: E402
import sampler_walk as sw  # noqa: E402

STAGES = ("kernel_build", "potrf", "trtri", "solve_alpha", "loo_q", "lauum", "lml_traces", "loo_mirror", "loo_gram", "loo_traces")


def evaluation(N, d, reps):
    model = sw.Model(d, sw.M52, N, seed=1)
    gpr = model.gpr()
    gpr._ensure_factor()
    dev = gpr.device
    theta = np.array(gpr.kernel_.device_spec(d)[1], dtype=float) + 0.05        # (away from the prediction factor's theta)
    calls = {"lml": lambda: dev.lml(theta, True), "loo_objective": lambda: dev.loo_objective(theta, True)}
    for f in calls.values():
        for _ in range(5):
            f()
    ms = {k: [] for k in calls}
    for _ in range(reps):                                   # alternating: both see the same machine
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(f"N={N} d={d}: one evaluation with gradient, wall per call over {reps} alternating calls: "
          + "; ".join(f"{k} median {med[k]:.3f} ms, best {min(ms[k]):.3f} ms, 90 % below {np.quantile(ms[k], 0.9):.3f} ms" for k in calls)
          + f"; ratio of the medians {med['loo_objective'] / med['lml']:.2f}", flush=True)
    for k, f in calls.items():                              # the stages, with the timers on
        dev.timing_reset()
        for _ in range(20):
            f()
        parts = {s: dev.timing(s) for s in STAGES}
        print(f"N={N} d={d}: {k}, device time per stage (mean of 20 calls, us): "
              + ", ".join(f"{s} {1e3 * t / c:.1f}" for s, (t, c) in parts.items() if c)
              + f"; sum {1e3 * sum(t / c for t, c in parts.values() if c):.1f}", flush=True)
    v, g, info = dev.loo_objective(theta, True)
    lml, gl, _ = dev.lml(theta, True)
    print(f"N={N} d={d}: loo value {v!r} (info {info}), LML {lml!r}; |grad| max {np.max(np.abs(g)):.4g} / {np.max(np.abs(gl)):.4g}", flush=True)


def fit_gpr(X, y, bounds, kernel, n_restarts, seed=5):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    g = GaussianProcessRegressor(kernel=kernel, bounds=bounds, n_restarts_optimizer=n_restarts, noise_level=1e-2,
                                 preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(),
                                 account_for_inf=None, random_state=seed)
    g.fit_lockstep = False          # the sequential loop on the model's own context for both objectives
    g.fit_devices = [0]
    return g


def full_fit(N, d, n_restarts):
    from gpry_amd.kernels import ConstantKernel as C, Matern, WhiteKernel
    model = sw.Model(d, sw.M52, N, seed=1)
    for objective in ("lml", "loo", "lml", "loo"):          # (the first pair warms both paths up)
        kernel = C(1.0, [1e-3, 1e4]) * Matern(np.ones(d), [1e-3, 10.], nu=2.5) + WhiteKernel(1e-2, [1e-6, 1e1])
        g = fit_gpr(model.X, model.y, model.bounds, kernel, n_restarts)
        g.append_to_data(model.X, model.y, fit_gpr=False)
        n0 = g.n_eval_loglike
        t0 = time.perf_counter()
        g.fit_gpr_hyperparameters(objective=objective)
        dt = time.perf_counter() - t0
        print(f"N={N} d={d}: sequential fit, {n_restarts} restarts, objective {objective}: {dt:.3f} s, {g.n_eval_loglike - n0} "
              f"evaluations, {1e3 * dt / (g.n_eval_loglike - n0):.3f} ms each; LML {g.log_marginal_likelihood_value_:.4f}, "
              f"leave-one-out {g.loo_log_predictive(g.kernel_.theta):.4f}; fit_stats {g.fit_stats}", flush=True)


def calibration(N=400, d=2, seed=3):
    """An RBF kernel on Matern-1/2-rough data: a draw of a GP with the exponential kernel plus a little noise."""
    from oracle import gpry_oracle as orc
    from gpry_amd.kernels import RBF, ConstantKernel as C, WhiteKernel
    from gpry_amd.mc import validate_gp
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, d))
    K = orc.kernel_matrix(X, np.log([1.0] + [0.5] * d), orc.MATERN12) + 1e-10 * np.eye(N)
    y = np.linalg.cholesky(K).dot(rng.standard_normal(N)) + 0.01 * rng.standard_normal(N)
    bounds = np.array([[0.0, 1.0]] * d)
    for objective in ("lml", "loo"):
        kernel = C(1.0, [1e-3, 1e4]) * RBF(np.ones(d), [1e-3, 10.]) + WhiteKernel(1e-2, [1e-8, 1e1])
        g = fit_gpr(X, y, bounds, kernel, 6)
        g.append_to_data(X, y, fit_gpr={"objective": objective})
        r = validate_gp(g).loo
        print(f"misspecified model (RBF + white on Matern-1/2 data, N={N}, d={d}), fitted by {objective}: kernel {g.kernel_}; "
              f"LML {g.log_marginal_likelihood_value_:.3f}, leave-one-out {g.loo_log_predictive(g.kernel_.theta):.3f}; "
              f"rms z {r['rms']:.3f}, |z| <= 1: {r['frac1']:.3f} (0.683), |z| <= 2: {r['frac2']:.3f} (0.954), "
              f"mean log density {r['mean_logpdf']:.4f}, {len(r['outliers'])} beyond 3", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024:8,4096:16")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--skip-fit", action="store_true")
    a = ap.parse_args()
    for spec in a.sizes.split(","):
        N, d = (int(v) for v in spec.split(":"))
        evaluation(N, d, a.reps)
    if not a.skip_fit:
        full_fit(1024, 8, 4)
        calibration()


if __name__ == "__main__":
    main()
