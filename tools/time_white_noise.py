#!/usr/bin/env python3
"""Timings of profiles/white_noise.md: one LML + gradient evaluation at (N, d) = (1024, 8) and (4096, 16) and a
``lml_batch`` of 32 thetas at 1024, without and (``--white``) with a fitted noise level; one JSON line per figure.

    python tools/time_white_noise.py TAG [--white]

Wall time per call around the Python method (every call ends in a stream synchronisation), 3 warm-up calls, then the median
of 300 / 60 / 40 calls.  To compare two builds, alternate them in one session: ``GPRY_HIP_LIB=<the other libgpry_hip.so>``
selects the library (a build without the flag is run without ``--white``).
"""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gpry_amd import _lib  # noqa: E402


def timeit(f, n, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), p90_ms=float(np.percentile(ts, 90)), n=n)


def main():
    tag, white = sys.argv[1], "--white" in sys.argv[2:]
    dev = _lib.Device(0)
    for N, d, n in ((1024, 8, 300), (4096, 16, 60)):
        rng = np.random.default_rng(N)
        X_ = rng.uniform(0, 1, (N, d))
        y_ = np.sin(3 * X_.sum(1)) + 0.1 * rng.standard_normal(N)
        theta = np.log(np.append(2.0, rng.uniform(0.3, 0.6, d)))
        dev.set_train(X_, y_, np.full(N, 1e-4))
        for flag in ((0, 1) if white else (0,)):
            lw = [math.log(0.05)] * flag
            dev.set_theta(3 | (_lib.KERNEL_WHITE if flag else 0), np.append(theta, lw))
            th = np.append(theta + 0.05, lw)
            print(json.dumps(dict(tag=tag, what="lml_grad", N=N, d=d, white=flag, **timeit(lambda: dev.lml(th, True), n))))
            if N == 1024:
                T = np.array([np.append(theta + 0.01 * k, [v + 0.01 * k for v in lw]) for k in range(32)])
                print(json.dumps(dict(tag=tag, what="lml_batch32", N=N, d=d, white=flag,
                                      **timeit(lambda: dev.lml_batch(T, True), 40))))
    dev.close()


if __name__ == "__main__":
    main()
