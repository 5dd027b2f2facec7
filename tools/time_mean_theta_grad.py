"""The derivative of the mean in theta on the device, timed: gpry_mean_theta_grad at M = 1024 and M = 65536 points on
config1's model (N = 1024, d = 8, RBF) and on the bench's (N = 4096, d = 16, Matern-5/2): device time and wall time of the
call, its split into setup and points from the two stage timers, the main kernel's L2 traffic against the chip's L2 rate,
and beside it the two routes there were before:
  (a) the numpy closed form on the fetched factor (timed on 1024 points; it is linear in M);
  (b) central differences through the device, 2 p x (set_theta, factorize, predict) -- what a user had to do.
Prints the rows and writes a markdown table.

    python tools/time_mean_theta_grad.py [--md profiles/mean_theta_grad_times.md] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools"), os.path.join(ROOT, "tools")]

L2_TBS = 17.0           # chip-wide L2 read rate, rows shared by every workgroup (lower end of the measured 16.8-18.8 TB/s)


def numpy_route(gpr, X, kid, theta, white):
    """Route (a): W from the fetched V and alpha_, then G, one coordinate at a time (memory O(M N))."""
    dev, d = gpr.device, gpr.d
    t0 = time.perf_counter()
    _, V, al = dev.get_factor(want_L=False)
    N = len(al)
    V = V[:N, :N]
    X_ = np.asarray(gpr.X_train_, dtype=float)
    C, ls = np.exp(theta[0]), np.exp(theta[1:d + 1])
    w = np.exp(theta[d + 1]) if white else 0.0
    noise = np.broadcast_to(gpr.alpha, (N,))

    def kernel_terms(A, B):
        D = [((A[:, a, None] - B[None, :, a]) / ls[a]) ** 2 for a in range(d)]
        r = np.sqrt(sum(D))
        with np.errstate(divide="ignore", invalid="ignore"):
            if kid == 0:
                phi = np.exp(-0.5 * r * r)
                h = phi
            elif kid == 1:
                phi = np.exp(-r)
                h = np.where(r > 0, phi / r, 0.0)
            elif kid == 2:
                phi, h = (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r), 3 * np.exp(-np.sqrt(3) * r)
            else:
                t = np.sqrt(5) * r
                phi, h = (1 + t + t * t / 3) * np.exp(-t), (5.0 / 3.0) * (1 + t) * np.exp(-t)
        return C * phi, C * h, D

    _, Ch, D = kernel_terms(X_, X_)
    U = np.stack([(noise + w) * al] + [(Ch * D[a]).dot(al) for a in range(d)] + ([w * al] if white else []), axis=1)
    Wm = V.T.dot(V.dot(U))
    Xq_ = gpr.preprocessing_X.transform(X)
    k, Ch, D = kernel_terms(Xq_, X_)
    G = np.empty((len(X), U.shape[1]))
    G[:, 0] = k.dot(Wm[:, 0])
    for a in range(d):
        G[:, 1 + a] = (Ch * D[a]).dot(al) - k.dot(Wm[:, 1 + a])
    if white:
        G[:, d + 1] = -k.dot(Wm[:, d + 1])
    G *= gpr._y_affine()[1]
    return G, 1e3 * (time.perf_counter() - t0)


def differences_route(dev, X, kid_flag, theta, h=1e-4):
    """Route (b): central differences through set_theta + factorize + predict; the model is put back afterwards."""
    t0 = time.perf_counter()
    G = np.empty((len(X), len(theta)))
    for j in range(len(theta)):
        vals = []
        for s in (1.0, -1.0):
            th = theta.copy()
            th[j] += s * h
            dev.set_theta(kid_flag, th)
            assert dev.factorize() == 0
            vals.append(dev.predict(X))
        G[:, j] = (vals[0] - vals[1]) / (2 * h)
    ms = 1e3 * (time.perf_counter() - t0)
    dev.set_theta(kid_flag, theta)
    assert dev.factorize() == 0
    return G, ms


def rows_for(name, gpr, bounds, reps):
    from gpry_amd import _lib
    from gpry_amd.mc import _push_model
    _push_model(gpr, "mean_theta_grad")
    dev, d = gpr.device, len(bounds)
    kid_flag, theta = gpr._device_theta()
    theta = np.asarray(theta, dtype=float)
    white = bool(kid_flag & _lib.KERNEL_WHITE)
    kid = kid_flag & 0xF
    N, p = dev.N, len(theta)
    dpad = (d + 1) & ~1
    rng = np.random.default_rng(0)
    rows = []
    for M in (1024, 65536):
        X = rng.uniform(bounds[:, 0], bounds[:, 1], (M, d))
        dev.mean_theta_grad(X)
        ms, wall, setup, main = [], [], [], []
        for _ in range(reps):
            dev.timing_reset()
            t0 = time.perf_counter()
            out = dev.mean_theta_grad(X)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(out["device_ms"])
            setup.append(dev.timing("theta_grad_setup")[0])
            main.append(dev.timing("theta_grad")[0])
        dev.set_option("timing", 0)
        G = out["G"]
        Ga, a_ms = numpy_route(gpr, X[:1024], kid, theta, white)
        Gd, b_ms = differences_route(dev, X, kid_flag, theta)
        again = dev.mean_theta_grad(X)["G"]
        assert np.array_equal(again, G), "the model was not put back"
        colmax = np.max(np.abs(Ga), axis=0)
        # the main kernel's reads per point: the pass of the value (a row and its alpha) and the pass of the gradient (a row,
        # its alpha, the row of W: the length-scale columns of the lanes' blocks and the line of the two extra entries)
        wcols = (16 if d <= 16 else 32) + 2
        bytes_pt = 8.0 * N * ((dpad + 1) + (dpad + 1 + wcols))
        l2_ms = 1e3 * M * bytes_pt / (L2_TBS * 1e12)
        row = dict(model=name, M=M, device_ms=float(np.median(ms)), wall_ms=float(np.median(wall)), setup_ms=float(np.median(setup)),
                   main_ms=float(np.median(main)), a_ms=a_ms, b_ms=b_ms, l2_ms=l2_ms,
                   dev_a=float(np.max(np.max(np.abs(G[:1024] - Ga), axis=0) / colmax)),
                   dev_b=float(np.max(np.max(np.abs(G - Gd), axis=0) / np.max(np.abs(G), axis=0))))
        print(f"{name}: M = {M}: call device {row['device_ms']:.3f} ms, wall {row['wall_ms']:.3f} ms (setup {row['setup_ms']:.3f}, "
              f"points {row['main_ms']:.3f}; L2 traffic at {L2_TBS} TB/s {l2_ms:.3f} ms = {100 * l2_ms / row['main_ms']:.0f} % of the "
              f"kernel's time); route (a) numpy on 1024 points {a_ms:.0f} ms; route (b) differences through the device "
              f"{b_ms:.0f} ms = {b_ms / row['wall_ms']:.1f} x the call; worst column deviation from (a) {row['dev_a']:.1e}, from (b) "
              f"{row['dev_b']:.1e}", flush=True)
        rows.append(row)
    return rows


def markdown(rows, device, reps):
    L = [f"Measured by `python tools/time_mean_theta_grad.py`, one {device}; medians of {reps} calls, warm context; routes (a) "
         "and (b) once each.", "",
         "| model | M | call: device ms | wall ms | setup ms | points ms | L2 traffic at 17 TB/s, ms (share of points) | (a) numpy, 1024 "
         "points, ms | (b) differences through the device, ms | (b) / call |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append(f"| {r['model']} | {r['M']} | {r['device_ms']:.3f} | {r['wall_ms']:.3f} | {r['setup_ms']:.3f} | {r['main_ms']:.3f} | "
                 f"{r['l2_ms']:.3f} ({100 * r['l2_ms'] / r['main_ms']:.0f} %) | {r['a_ms']:.0f} | {r['b_ms']:.0f} | "
                 f"{r['b_ms'] / r['wall_ms']:.1f} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from time_maximize import models
    rows, device = [], None
    for name, gpr, bounds in models():
        device = gpr.device.info()["arch"]
        rows += rows_for(name, gpr, bounds, args.reps)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(rows, device, args.reps))


if __name__ == "__main__":
    main()
