#!/usr/bin/env python3
"""Dump what ``run_nested`` of one source tree computes on the numpy stand-in devices of tests/tools, to compare two trees'
host bookkeeping bit for bit on one machine (numpy's exp / log differ between CPUs: never compare across hosts).

    python tools/dump_nested_host.py TREE_A a.npz
    python tools/dump_nested_host.py TREE_B b.npz
    python tools/dump_nested_host.py --compare a.npz b.npz

A two-mode Gaussian in d = 2, nlive 40, num_repeats 4, seeds 1 and 2, nprior 40 and 100, in four modes: plain;
clustering; clustering with cluster_volumes; phantom_thin 2.  Every field of the NestedResult but wall_s is stored;
``--compare`` asks np.array_equal of every array (scalars are stored as 0-d arrays) and exits 1 on a difference."""
import os
import sys

import numpy as np

MODES = {"plain": ("ns_philox", "NumpyNestedDevice", {}),
         "clustering": ("ns_cluster", "ClusteredNumpyDevice", {"clustering": True}),
         "volumes": ("ns_volumes", "VolumesNumpyDevice", {"clustering": True, "cluster_volumes": True}),
         "phantoms": ("ns_phantoms", "PhantomNumpyDevice", {"phantom_thin": 2})}


def loglike(X):
    X = np.atleast_2d(X)
    a = -0.5 * np.sum((X - np.array([-2.0, 0.5])) ** 2, axis=1) / 0.3 ** 2
    b = -0.5 * np.sum((X - np.array([2.0, -0.5])) ** 2, axis=1) / 0.4 ** 2
    return np.logaddexp(a, b + np.log(0.5))


def dump(tree, out):
    sys.path[:0] = [tree, os.path.join(tree, "tests", "tools")]
    from gpry_amd.nested import run_nested
    bounds = np.array([[-4.0, 4.0]] * 2)
    res = {}
    for mode, (module, cls, kw) in MODES.items():
        device = getattr(__import__(module), cls)
        for seed in (1, 2):
            for nprior in (40, 100):
                r = run_nested(device(loglike), bounds, seed, 40, 4, nprior=nprior, **kw)
                for name, v in r._asdict().items():
                    if name != "wall_s" and v is not None:
                        res[f"{mode}/{seed}/{nprior}/{name}"] = np.asarray(v)
                print(f"{mode}, seed {seed}, nprior {nprior}: {r.ngen} generations, {len(r.y)} rows, logZ {r.logZ!r}")
    np.savez(out, **res)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k])]
    print(f"{len(A.files)} arrays, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(os.path.abspath(sys.argv[1]), sys.argv[2]))
