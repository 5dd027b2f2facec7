"""The Kriging-believer ranking in C++ (gpry_amd/csrc/kb_rank_core.h, what gpry_kb_rank runs on the host) against the
Python RankedPool, without a GPU: a host-only shim (tests/c_abi/kb_rank_host.cpp) is compiled with the system C++ compiler
and driven through ctypes with Gram rows from the oracle device double's session."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import attach

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kb_rank_common as kc  # noqa: E402

GRAM_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("kb_rank") / "kb_rank_host.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "gpry_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "kb_rank_host.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.kb_rank_host.restype = C.c_int64
    lib.kb_rank_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), GRAM_FN, C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def make_gpr(bounds, theta, noise_level):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import clone
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    gpr = attach(GaussianProcessRegressor(kernel={"Matern": {"nu": 2.5}}, bounds=bounds, noise_level=noise_level,
                                          preprocessing_X=Normalize_bounds(bounds), preprocessing_y=Normalize_y(),
                                          account_for_inf=None))
    k = clone(gpr.kernel)
    k.theta = theta
    gpr.kernel_, gpr._fitted = k, True
    return gpr


class ShimPool:
    """The pool's arrays as the shim keeps them, fed with the offers the Python pool got."""

    def __init__(self, lib, gpr, n, f):
        self.lib, self.gpr, self.n, self.f = lib, gpr, n, f
        self.idx = np.full(n + 1, -1, dtype=np.int64)
        self.y, self.sigma, self.acq = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
        self.acq_cond = np.full(n + 1, -np.inf)
        self.cache_counter = 0
        self.stats = np.zeros(2, dtype=np.int64)

    def add(self, X, y, sigma, acq, speculative=None):
        sess = self.gpr.kb_session()
        idx = sess.register(X)
        n_s = sess.n
        var0 = np.ascontiguousarray(sess.var0, dtype=float)

        def gram(user, p, G, kv):
            g, k = sess.gram(int(p))
            np.ctypeslib.as_array(G, (n_s,))[:] = g
            np.ctypeslib.as_array(kv, (n_s,))[:] = k

        kw = self.f.keywords
        params = np.array([kw["noise_level"], sess.noise_alpha(), kw["baseline"], kw["zeta"], sess.std_y], dtype=float)
        order = np.ascontiguousarray(np.argsort(acq)[::-1], dtype=np.int64)
        y, sigma, acq = (np.ascontiguousarray(a, dtype=float) for a in (y, sigma, acq))
        counter = C.c_int64(self.cache_counter)
        spec = 2 * self.n if speculative is None else speculative
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        info = self.lib.kb_rank_host(n_s, p(var0), p(idx), p(y), p(sigma), p(acq), len(idx), p(order), len(order),
                                     p(params), self.n, p(self.idx), p(self.y), p(self.sigma), p(self.acq),
                                     p(self.acq_cond), C.byref(counter), GRAM_FN(gram), None, spec, p(self.stats))
        assert info >= 0, info
        self.cache_counter = counter.value
        self.X = np.where((self.idx >= 0)[:, None], sess.X[np.maximum(self.idx, 0)], 0.0)
        return info


# (N, d) x n_points x offers of 8 to 300 rows: the seeds were chosen on the CPU so that conditioning reorders the pool in
# at least half of the cases and a near-tie inside one sort of the Python path is met in at most 5 %
CASES = [(N, d, n_points, M, seed)
         for N in (20, 130) for d in (2, 5) for n_points in (1, 3, 8, 16)
         for M, seed in ((8, 1), (37, 2), (120, 3), (300, 4))]


def _run_case(shim, N, d, n_points, M, seed, feeds=1, duplicates=False, speculative=None):
    bounds, gpr = kc.long_scale_model(make_gpr, N, d, seed=100 + seed)
    Xc, ym, sm, a, f = kc.offer(gpr, bounds, M, seed)
    if duplicates:
        dup = np.arange(0, M, 3)
        Xc, ym, sm, a = (np.concatenate([v, v[dup]]) for v in (Xc, ym, sm, a))
    ref = kc.TrackedPool(n_points, gpr=gpr, acq_func=f, verbose=0)
    parts = np.array_split(np.arange(len(Xc)), feeds)
    with np.errstate(divide="ignore"):
        for part in parts:
            ref.add(Xc[part], ym[part], sm[part], a[part], method="single sort acq")
    gpr._kb = None      # (a session of its own for the shim: same rows, same bits)
    mine = ShimPool(shim, gpr, n_points, f)
    for part in parts:
        assert mine.add(Xc[part], ym[part], sm[part], a[part], speculative=speculative) == 0
    return ref, mine, [a[part] for part in parts]


def test_the_shim_ranks_as_the_python_pool_over_random_models(shim):
    n_reordered = n_tied = 0
    for N, d, n_points, M, seed in CASES:
        ref, mine, offers = _run_case(shim, N, d, n_points, M, seed)
        if ref.near_tie:
            n_tied += 1
            continue
        n_reordered += kc.reordered(ref, offers)
        kc.assert_same_ranking(mine, ref, f"N={N} d={d} n_points={n_points} M={M}")
    print(f"{len(CASES)} cases, {n_reordered} reordered, {n_tied} with a near-tie")
    assert n_tied <= 0.05 * len(CASES)
    assert n_reordered >= 0.5 * len(CASES)


@pytest.mark.parametrize("speculative", [-1, 0])
def test_rows_in_front_or_on_demand_give_the_same_pool(shim, speculative):
    ref, mine, _ = _run_case(shim, 130, 5, 8, 120, 3, speculative=speculative)
    kc.assert_same_ranking(mine, ref)
    if speculative == 0:
        assert mine.stats[1] >= 1      # the core asked for rows itself


def test_duplicate_rows_in_an_offer(shim):
    ref, mine, _ = _run_case(shim, 20, 2, 8, 37, 2, duplicates=True)
    assert not ref.near_tie
    kc.assert_same_ranking(mine, ref)


def test_an_offer_fed_in_two_calls(shim):
    ref, mine, offers = _run_case(shim, 130, 2, 8, 120, 3, feeds=2)
    assert not ref.near_tie
    kc.assert_same_ranking(mine, ref)
    assert kc.reordered(ref, offers)


def test_the_walk_ends_at_the_admission_level(shim):
    """A second offer whose values are all at or below the pool's admission level: the walk breaks at its first row,
    nothing is touched, no model is built and no Gram row is asked for."""
    bounds, gpr = kc.long_scale_model(make_gpr, 20, 5, seed=102)
    Xc, ym, sm, a, f = kc.offer(gpr, bounds, 60, 2)
    first, second = np.arange(40), np.arange(40, 60)
    ref = kc.TrackedPool(3, gpr=gpr, acq_func=f, verbose=0)
    ref.add(Xc[first], ym[first], sm[first], a[first], method="single sort acq")
    low = ref.min_acq - np.arange(len(second), dtype=float)       # the best one EQUAL to the admission level
    counter = ref.cache_counter
    ref.add(Xc[second], ym[second], sm[second], low, method="single sort acq")
    assert ref.cache_counter == counter
    gpr._kb = None
    mine = ShimPool(shim, gpr, 3, f)
    assert mine.add(Xc[first], ym[first], sm[first], a[first]) == 0
    assert mine.add(Xc[second], ym[second], sm[second], low, speculative=0) == 0
    assert tuple(mine.stats) == (0, 0)
    kc.assert_same_ranking(mine, ref)


def test_a_point_that_breaks_positive_definiteness_gives_the_python_error(shim, monkeypatch):
    """The Gram row of one accepted offer claims |u(p)|^2 > k(p, p): the border of the model that takes it in is not
    positive definite.  Both paths see the same rows and stop at the same appended point."""
    from gpry_amd.kriging import KBSession
    bounds, gpr = kc.long_scale_model(make_gpr, 20, 2, seed=105)
    Xc, ym, sm, a, f = kc.offer(gpr, bounds, 37, 5)
    clean = kc.TrackedPool(8, gpr=gpr, acq_func=f, verbose=0)
    clean.add(Xc, ym, sm, a, method="single sort acq")
    # the candidate an undisturbed ranking leaves in slot 2 (offers without duplicates: session index = row)
    p_bad = int(np.flatnonzero(np.all(Xc == clean.X[2], axis=1))[0])
    gpr._kb = None
    real = KBSession.gram

    def gram(self, p):
        G, kv = real(self, p)
        if p == p_bad:
            G = G.copy()
            G[p_bad] = kv[p_bad] + 1.0
        return G, kv

    monkeypatch.setattr(KBSession, "gram", gram)
    ref = kc.TrackedPool(8, gpr=gpr, acq_func=f, verbose=0)
    with pytest.raises(np.linalg.LinAlgError) as err:
        ref.add(Xc, ym, sm, a, method="single sort acq")
    gpr._kb = None
    mine = ShimPool(shim, gpr, 8, f)
    info = mine.add(Xc, ym, sm, a)
    assert info >= 2
    assert str(err.value) == (f"{info}-th appended point makes the augmented kernel matrix non positive definite. Try "
                              "gradually increasing the 'noise_level' parameter of your GaussianProcessRegressor "
                              "estimator.")
