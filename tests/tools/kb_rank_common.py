"""What tests/test_kb_rank_cpu.py and tests/test_kb_rank_gpu.py share: models whose length scales are long enough that
Kriging-believer conditioning reorders a pool, a RankedPool that notes near-ties inside ``sort``, and the comparison of a
native ranking with the Python path."""
from functools import partial
from unittest import mock

import numpy as np

from gpry_amd.acquisition_functions import LogExp
from gpry_amd.gp_acquisition import RankedPool

TIE_RTOL = 1e-10


class TrackedPool(RankedPool):
    """The Python path, noting whether one ``sort`` met two conditioned values within TIE_RTOL (a tie that numpy's sort
    may break either way: such a case says nothing about the native ranking)."""

    near_tie = False

    def sort(self, i_start=0):
        real = np.argsort

        def argsort(a, *args, **kw):
            v = np.sort(np.asarray(a, dtype=float)[np.isfinite(a)])
            if len(v) > 1 and np.any(np.diff(v) <= TIE_RTOL * np.maximum(np.abs(v[1:]), np.abs(v[:-1]))):
                self.near_tie = True
            return real(a, *args, **kw)

        with mock.patch.object(np, "argsort", argsort):
            return super().sort(i_start)


def long_scale_model(make_gpr, N, d, seed, scale=3.0, noise_level=1e-2):
    """A GPR (Matern-5/2) on N points of a correlated Gaussian in d dimensions with length scales of `scale` box widths --
    every candidate is strongly correlated with every other, so accepting one moves the conditioned values of the rest."""
    from oracle import gpry_oracle as orc
    bounds, X, y, _ = orc.synthetic_like_goldens(N, d, 1, seed=seed)
    theta = np.log(np.array([4.0] + [scale] * d))
    gpr = make_gpr(bounds, theta, noise_level)
    gpr.append_to_data(X, y, fit_gpr=False)
    return bounds, gpr


def offer(gpr, bounds, M, seed):
    rng = np.random.default_rng(seed)
    Xc = rng.uniform(bounds[:, 0], bounds[:, 1], size=(M, len(bounds)))
    ym, sm = gpr.predict(Xc, return_std=True)
    f = partial(LogExp.f, baseline=gpr.y_max, noise_level=gpr.noise_level, zeta=len(bounds) ** -0.85)
    with np.errstate(divide="ignore"):
        return Xc, ym, sm, f(ym, sm), f


def filled(pool):
    return int(np.count_nonzero(pool.acq_cond[:-1] > -np.inf))


def reordered(pool, offers_acq):
    """The final order is not the plain descending-acquisition order of what was offered."""
    k = filled(pool)
    return not np.array_equal(pool.acq[:k], np.sort(np.concatenate(offers_acq))[::-1][:k])


def assert_same_ranking(native, ref, what=""):
    """The three assertions: picks and their order, cache_counter, acq_cond to 1e-12."""
    k = filled(ref)
    assert filled(native) == k, what
    np.testing.assert_array_equal(native.X[:k], ref.X[:k], err_msg=f"picks {what}")
    for name in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(getattr(native, name)[:k], getattr(ref, name)[:k], err_msg=f"{name} {what}")
    assert native.cache_counter == ref.cache_counter, what
    np.testing.assert_allclose(native.acq_cond[:k], ref.acq_cond[:k], rtol=1e-12, atol=0, err_msg=f"acq_cond {what}")
    assert np.all(native.acq_cond[k:] == -np.inf), what
