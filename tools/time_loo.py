"""Device and wall time of Device.loo and Device.leave_out (the partition into batches of 4; 64 groups of 64) on config1
(N = 1024, d = 8) and at N = 4096, d = 16, beside the numpy route (get_factor, then tests/tools/loo_numpy.py, the fetch
included): the tables of profiles/loo.md.  ``--once``: three warmed calls of each and nothing else (for a kernel trace: the
time of loo_pass_kernel alone over the bytes of V's lower triangle is the achieved rate of the pass)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np  # noqa: E402
import loo_numpy as ln  # noqa: E402
import sampler_walk as sw  # noqa: E402

HBM_STREAM = (6.5e12, 6.9e12)       # bytes/s the box was measured to stream (tools/r04/hbm_ceiling.hip)


def timed(f, reps, warm=3):
    for _ in range(warm):
        f()
    ms, t0 = [], time.perf_counter()
    for _ in range(reps):
        ms.append(f()["device_ms"])
    wall = (time.perf_counter() - t0) / reps * 1e3
    return float(np.median(ms)), float(np.min(ms)), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024:8,4096:16")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    for spec in a.sizes.split(","):
        N, d = (int(v) for v in spec.split(":"))
        model = sw.Model(d, sw.M52, N, seed=1)
        gpr = model.gpr()
        gpr._ensure_factor()
        gpr._push_affine()
        dev = gpr.device
        rng = np.random.default_rng(0)
        part = [np.arange(k, min(k + 4, N)) for k in range(0, N, 4)]
        big = [rng.choice(N, 64, replace=False) for _ in range(64)]
        if a.once:
            for _ in range(3):
                dev.loo()
                dev.leave_out(part)
                dev.leave_out(big)
            continue
        tri = 8 * N * (N + 1) // 2
        tiles = ((N + 63) // 64) * ((N + 63) // 64 + 1) // 2 * 64 * 64 * 8
        med, best, wall = timed(dev.loo, a.reps)
        print(f"N={N} d={d}: loo device {med:.4f} ms median, {best:.4f} ms best, wall {wall:.4f} ms per call ({a.reps} calls); "
              f"lower triangle of V {tri / 1e6:.1f} MB ({tiles / 1e6:.1f} MB in whole tiles): the whole call, finish and copies "
              f"included, moves {tri / (best * 1e-3) / 1e12:.3f} TB/s = {100 * tri / (best * 1e-3) / HBM_STREAM[1]:.1f}-"
              f"{100 * tri / (best * 1e-3) / HBM_STREAM[0]:.1f} % of the streaming rate", flush=True)
        for name, groups in (("partition into batches of 4", part), ("64 groups of 64", big)):
            med, best, wall = timed(lambda: dev.leave_out(groups), max(a.reps // 10, 5))
            print(f"N={N} d={d}: leave_out, {name} ({len(groups)} groups): device {med:.4f} ms median, {best:.4f} ms best, "
                  f"wall {wall:.4f} ms per call", flush=True)
        y_mean, y_std = gpr._y_affine()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, V, al = dev.get_factor(want_L=False)
            t1 = time.perf_counter()
            ln.loo(V, al, gpr.y_train_, gpr.alpha, y_mean, y_std)
            t2 = time.perf_counter()
            ln.leave_out(V, al, gpr.y_train_, big, y_mean, y_std)
            t3 = time.perf_counter()
            t.append((t1 - t0, t2 - t1, t3 - t2))
        f, l, g = (1e3 * float(np.median([r[k] for r in t])) for k in range(3))
        print(f"N={N} d={d}: numpy route: get_factor (V, alpha_) {f:.1f} ms, loo_numpy.loo {l:.1f} ms, "
              f"leave_out of 64 groups of 64 {g:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
