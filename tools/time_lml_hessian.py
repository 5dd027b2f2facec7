"""The measurements of profiles/lml_hessian.md: one ``gpry_lml_hessian`` (device time and wall time of the call), its split
by stage through the library's stage timers (a run of their own: the timers add two events per stage) with the GEMM engine's
rate in the batched product, and beside it -- in the same run, on the same model -- the two ways to the same Hessian that
exist without the entry point: central differences from 2p calls of ``dev.lml(theta +- h e_j, True)`` (h = 1e-5), with their
deviation from the device Hessian, and the numpy closed form on the factor fetched from the device.  Sizes: config1's model
(N = 1024, d = 8, RBF) and N = 4096, d = 16, Matern-5/2.

One process; every GPU step runs under a time limit of its own (``--limit`` seconds): a watchdog thread that ends the whole
process when the step has not come back by then -- also where the step sits inside a library call and the interpreter
never gets to run a signal handler -- so nothing is started on the device after a step that ran over."""
import argparse
import os
import threading
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np  # noqa: E402
import sampler_walk as sw  # noqa: E402
import lml_hessian_model as hm  # noqa: E402

STAGES = ("kernel_build", "potrf", "trtri", "solve_alpha", "lauum", "lml_traces", "hess_pairs", "hess_products", "hess_btraces",
          "hess_middle", "hess_finish")


def step(name, limit, f):
    """f() under a watchdog of `limit` seconds; a step that runs into it ends the process (exit status 3)."""
    def expired():
        print(f"step '{name}' ran into its limit of {limit} s: stopping, nothing more is started", flush=True)
        os._exit(3)
    guard = threading.Timer(limit, expired)
    guard.daemon = True
    guard.start()
    try:
        return f()
    finally:
        guard.cancel()


def closed_form_on_factor(X_, theta, kid, V, al):
    """hessian_via_V's arithmetic on the inverse factor V and alpha_ the device holds (no white term)."""
    from oracle import gpry_oracle as orc
    d = X_.shape[1]
    _, dK = orc.kernel_matrix(X_, theta, kid, eval_gradient=True)
    dKs = [dK[:, :, j] for j in range(d + 1)]
    W = np.outer(al, al) - V.T.dot(V)
    WCg, D = hm.second_weight(X_, theta, kid)
    WCg *= W
    grad = [0.5 * np.sum(W * k) for k in dKs]

    def first(i, j):        # (the second derivatives one at a time: 136 matrices of N^2 at d = 16 would not fit)
        if i == 0:
            return grad[j]
        return 0.5 * np.sum(WCg * D[:, :, i - 1] * D[:, :, j - 1]) - (2.0 * grad[i] if i == j else 0.0)
    A = [V.dot(k).dot(V.T) for k in dKs]
    u = [V.dot(k.dot(al)) for k in dKs]
    return hm._assemble(d + 1, first, lambda i, j: u[i].dot(u[j]), lambda i, j: np.sum(A[i] * A[j]))


def measure(N, d, kid, reps, limit, h=1e-5):
    tag = f"N={N} d={d} kernel {kid}"
    model = sw.Model(d, kid, N, seed=1)
    gpr = model.gpr()
    step("factorise", limit, gpr._ensure_factor)
    dev = gpr.device
    theta = np.array(gpr.kernel_.device_spec(d)[1], dtype=float)
    p = len(theta)
    Np = (N + 127) // 128 * 128

    def hessian_calls():
        for _ in range(3):
            dev.lml_hessian(theta)
        wall, devms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = dev.lml_hessian(theta)
            wall.append((time.perf_counter() - t0) * 1e3)
            devms.append(r["device_ms"])
        return r, wall, devms
    r, wall, devms = step("lml_hessian", limit, hessian_calls)
    print(f"{tag}: one lml_hessian over {reps} calls: device_ms median {np.median(devms):.3f}, best {min(devms):.3f}; wall median "
          f"{np.median(wall):.3f} ms, best {min(wall):.3f} ms; info {r['info']}", flush=True)

    def stages():
        dev.timing_reset()
        n = max(3, reps // 2)
        for _ in range(n):
            dev.lml_hessian(theta)
        return {s: dev.timing(s) for s in STAGES}
    parts = step("stages", limit, stages)
    print(f"{tag}: device time per stage (mean, us): " + ", ".join(f"{s} {1e3 * t / c:.1f}" for s, (t, c) in parts.items() if c)
          + f"; sum {1e3 * sum(t / c for t, c in parts.values() if c):.1f}", flush=True)
    t, c = parts["hess_products"]
    if c:
        print(f"{tag}: stage (c), {d} products of {Np}^3 in one launch: {d * 2.0 * Np ** 3 / (t / c * 1e-3) / 1e12:.1f} TFLOP/s", flush=True)

    def differences():
        for _ in range(3):
            dev.lml(theta, True)
        t0 = time.perf_counter()
        H = np.empty((p, p))
        for j in range(p):
            e = np.zeros(p)
            e[j] = h
            H[:, j] = (dev.lml(theta + e, True)[1] - dev.lml(theta - e, True)[1]) / (2.0 * h)
        return 0.5 * (H + H.T), (time.perf_counter() - t0) * 1e3
    Hfd, ms_fd = step("central differences", limit, differences)
    big = np.max(np.abs(r["H"]))
    print(f"{tag}: central differences, {2 * p} calls of lml with gradient, h = {h:g}: {ms_fd:.3f} ms wall; deviation from the "
          f"device Hessian {np.max(np.abs(Hfd - r['H'])) / big:.2e} of max|H|", flush=True)

    L, V, al = step("get_factor", limit, dev.get_factor)
    V, al = np.asarray(V)[:N, :N], np.asarray(al)[:N]
    t0 = time.perf_counter()
    Hnp = closed_form_on_factor(gpr.X_train_, theta, kid, V, al)
    ms_np = (time.perf_counter() - t0) * 1e3
    print(f"{tag}: numpy closed form on the fetched factor ({os.cpu_count()} CPUs visible): {ms_np:.0f} ms; deviation from the "
          f"device Hessian {np.max(np.abs(Hnp - r['H'])) / big:.2e} of max|H|", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024:8:0,4096:16:3", help="N:d:kernel id, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    a = ap.parse_args()
    for spec in a.sizes.split(","):
        N, d, kid = (int(v) for v in spec.split(":"))
        measure(N, d, kid, a.reps, a.limit)


if __name__ == "__main__":
    main()
