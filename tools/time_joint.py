"""Device and wall time of Device.predict_cov and Device.sample_joint (S = 256) at N = 4096, d = 16, beside the host route
(numpy K** - U^T U from the fetched V, np.linalg.cholesky, standard_normal @ L.T): the table of profiles/joint.md.
``--once m``: one warmed call of each at m points and nothing else (for a kernel trace)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np  # noqa: E402
import joint_numpy as jn  # noqa: E402
import sampler_walk as sw  # noqa: E402


def timed(f, reps):
    f()
    f()
    ms, t0 = [], time.perf_counter()
    for _ in range(reps):
        ms.append(f()["device_ms"])
    return float(np.median(ms)), (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    model = sw.Model(a.d, sw.M52, a.N, seed=1)
    gpr = model.gpr()
    gpr._ensure_factor()
    gpr._push_affine()
    dev = gpr.device
    rng = np.random.default_rng(0)
    for m in ([a.once] if a.once else [512, 4096]):
        X = np.ascontiguousarray(rng.uniform(-3.0, 3.0, (m, a.d)))
        if a.once:
            for _ in range(3):
                dev.predict_cov(X)
                dev.sample_joint(X, a.S, 1)
            continue
        reps = 20 if m <= 512 else 5
        c_dev, c_wall = timed(lambda: dev.predict_cov(X), reps)
        s_dev, s_wall = timed(lambda: dev.sample_joint(X, a.S, 1), reps)
        eps = dev.sample_joint(X, a.S, 1)["jitter_used"]
        # host route on the same box
        _, V, _ = dev.get_factor(want_L=False, want_alpha=False)
        X_ = gpr.preprocessing_X.transform(X) if gpr.preprocessing_X is not None else X
        y_std = float(gpr._y_affine()[1])
        t0 = time.perf_counter()
        Sg = jn.cov(X_, gpr.X_train_, model.theta, model.kid, V, y_std)
        t1 = time.perf_counter()
        L = np.linalg.cholesky(Sg + eps * np.exp(model.theta[0]) * y_std ** 2 * np.eye(m))
        t2 = time.perf_counter()
        np.random.default_rng(1).standard_normal((a.S, m)) @ L.T
        t3 = time.perf_counter()
        print(f"N={a.N} d={a.d} m={m}: predict_cov device {c_dev:.3f} ms, wall {c_wall:.3f} ms | sample_joint(S={a.S}) device "
              f"{s_dev:.3f} ms, wall {s_wall:.3f} ms (jitter_used {eps:g}) | host: cov {1e3 * (t1 - t0):.1f} ms, cholesky "
              f"{1e3 * (t2 - t1):.1f} ms, draws {1e3 * (t3 - t2):.1f} ms (V fetch not counted)", flush=True)


if __name__ == "__main__":
    main()
