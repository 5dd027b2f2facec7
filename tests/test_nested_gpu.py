"""The nested sampler of the surrogate on the device (gpry_amd/csrc/nested.hip + gpry_amd/nested.py): the prior draws equal
the numpy Philox restatement bit for bit; every returned y equals gpr.predict of its row bit for bit (nsplit 1, 4 and 8,
Normalize_bounds / Normalize_y, the clip, the SVM classifier with a trust region); the generations keep their invariants;
the same seed gives the same bits on one context and on another; the evidence and the posterior moments of fitted
surrogates agree with a quadrature of gpr.predict; NORA.multi_add(sampler="nested") agrees with the oracle's ranking of
the same pool with y given."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import gpry_oracle as orc
from test_given_y_cpu import oracle_given
from test_host_mirror_gpu import make_gpr

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_philox  # noqa: E402

pytestmark = pytest.mark.gpu


class Recorder:
    """Passes the two sampler calls through to the device and keeps what each generation returned."""

    def __init__(self, dev):
        self.dev, self.gens = dev, []

    def ns_prior(self, *a):
        return self.dev.ns_prior(*a)

    def ns_generation(self, lo, hi, Xs, ys, lstar, W, seed, gen, k, R):
        out = self.dev.ns_generation(lo, hi, Xs, ys, lstar, W, seed, gen, k, R)
        self.gens.append(dict(lstar=lstar, X=out[0], y=out[1], ncalls=out[2]))
        return out


def _gauss_ll(d, s=0.5, mu=0.3):
    return lambda X: -0.5 * np.sum((np.atleast_2d(X) - mu) ** 2, axis=1) / s ** 2


def _banana_ll(X):
    X = np.atleast_2d(X)
    return -0.5 * (X[:, 0] ** 2 / 1.0 + (X[:, 1] - 0.5 * X[:, 0] ** 2 + 0.5) ** 2 / 0.3 ** 2)


def _training(ll, d, N, seed, width=4.0, spread=1.0):
    """Half uniform on the box [-width, width]^d, half around the mode."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-width, width, (N // 2, d)),
                        np.clip(rng.normal(0.0, spread, (N - N // 2, d)), -width, width)])
    return np.array([[-width, width]] * d), X, ll(X)


def _fitted(ll, d, N, seed=0, **kw):
    bounds, X, y = _training(ll, d, N, seed)
    gpr = make_gpr(bounds, orc.MATERN52, n_restarts_optimizer=1, random_state=1, **kw)
    gpr.append_to_data(X, y, fit_gpr=True)
    return gpr, bounds


def _fixed(ll, d, N, theta, seed=0, **kw):
    bounds, X, y = _training(ll, d, N, seed)
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.asarray(theta, dtype=float), **kw)
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


def _run(gpr, bounds, seed, nlive, num_repeats, rec=False, **kw):
    from gpry_amd.nested import run_nested
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    dev = Recorder(gpr.device) if rec else gpr.device
    r = run_nested(dev, bounds, seed, nlive, num_repeats, minus_inf_value=gpr.minus_inf_value, **kw)
    return (r, dev) if rec else r


def _one_point(gpr, X):
    return np.array([gpr.predict(x[None, :], validate=False)[0] for x in X])


def test_prior_points_equal_the_numpy_restatement():
    gpr, bounds = _fixed(_gauss_ll(5), 5, 300, np.log([4.0] + [0.3] * 5))
    gpr._ensure_factor()
    gpr._push_affine()
    lo, hi = np.array([-4.0, -3.0, 0.5, -1e-3, 10.0]), np.array([4.0, 1.0, 0.75, 2e-3, 1e4])
    for seed in (0, 12345, 2**31 - 2):
        X, y, _ = gpr.device.ns_prior(lo, hi, seed, 3000)
        np.testing.assert_array_equal(X, ns_philox.prior_points(lo, hi, seed, 3000))
        assert np.all((X >= lo) & (X <= hi))
        np.testing.assert_array_equal(y[:200], _one_point(gpr, X[:200]))


def _parity_cases():
    yield "N=600 d=3 (nsplit 1)", lambda: _fixed(_gauss_ll(3), 3, 600, np.log([4.0, 0.3, 0.3, 0.3]))
    yield "N=4096 d=16 (nsplit 4)", lambda: _fixed(_gauss_ll(16, s=1.5), 16, 4096, np.log([4.0] + [0.3] * 16))
    yield "N=8300 d=4 (nsplit 8)", lambda: _fixed(_gauss_ll(4), 4, 8300, np.log([4.0] + [0.2] * 4))
    yield "clip active", lambda: _fixed(_gauss_ll(3), 3, 400, np.log([4.0, 0.3, 0.3, 0.3]), clip_factor=1.0)
    yield "SVM + trust region", lambda: _svm_model()


def _svm_model():
    ll = _gauss_ll(3)
    bounds, X, y = _training(ll, 3, 300, 9)
    y = y.copy()
    y[X[:, 0] > 1.5] = -np.inf
    gpr = make_gpr(bounds, orc.MATERN52, theta=np.log([4.0, 0.3, 0.3, 0.3]), account_for_inf="SVM",
                   inf_threshold="20s", trust_region_factor=1.5, random_state=1)
    gpr.append_to_data(X, y, fit_gpr=False)
    return gpr, bounds


@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_row_equals_one_point_predict(case):
    make = dict(_parity_cases())[case]
    gpr, bounds = make()
    r, rec = _run(gpr, bounds, 77, nlive=60, num_repeats=3, rec=True, nprior=240, max_ncalls=20000)
    assert len(r.y) > 60
    np.testing.assert_array_equal(r.y, _one_point(gpr, r.X))
    assert np.all((r.X >= bounds[:, 0]) & (r.X <= bounds[:, 1]))
    assert np.all(r.dead_L[1:] >= r.dead_L[:-1])
    if case == "SVM + trust region":
        # some of the prior fell on rejected ground; none of it is in the pool
        assert r.n_dead + 60 > len(r.y)
    if case != "clip active":          # (at the clip, ties make y = L* possible for a chain that never moved)
        for g in rec.gens:
            assert np.all(g["y"] > g["lstar"])
    # the run stops within one generation of max_ncalls
    last = int(np.sum(rec.gens[-1]["ncalls"])) if rec.gens else 0
    assert r.ncalls - 20000 <= last


def test_same_seed_same_bits_on_two_contexts():
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, theta)
    a = _run(gpr, bounds, 5, nlive=80, num_repeats=8, nprior=400)
    b = _run(gpr, bounds, 5, nlive=80, num_repeats=8, nprior=400)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)      # its own context
    assert gpr2.device is not gpr.device
    c = _run(gpr2, bounds, 5, nlive=80, num_repeats=8, nprior=400)
    for o in (b, c):
        np.testing.assert_array_equal(o.X, a.X)
        np.testing.assert_array_equal(o.y, a.y)
        np.testing.assert_array_equal(o.w, a.w)
        assert o.logZ == a.logZ and o.ncalls == a.ncalls
    e = _run(gpr, bounds, 6, nlive=80, num_repeats=8, nprior=400)
    assert not np.array_equal(e.X[:50], a.X[:50])


def _quadrature(gpr, bounds, n):
    """Midpoint grid of n^d cells through predict's large-M path: logZ, mean and covariance of exp(y)."""
    d = len(bounds)
    axes = [bounds[k, 0] + (np.arange(n) + 0.5) * (bounds[k, 1] - bounds[k, 0]) / n for k in range(d)]
    G = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    y = np.concatenate([gpr.predict(G[i:i + 500_000]) for i in range(0, len(G), 500_000)])
    m = np.max(y)
    p = np.exp(y - m)
    logZ = m + np.log(np.mean(p))
    p /= p.sum()
    mean = p @ G
    cov = (G - mean).T @ ((G - mean) * p[:, None])
    return logZ, mean, cov


@pytest.mark.timeout(900)
@pytest.mark.parametrize("target", ["gauss d=2", "gauss d=4", "banana d=2"])
def test_evidence_and_moments_against_quadrature(target):
    if target == "gauss d=2":
        gpr, bounds = _fitted(_gauss_ll(2), 2, 200)
        n = 400
    elif target == "gauss d=4":
        gpr, bounds = _fitted(_gauss_ll(4), 4, 400)
        n = 40
    else:
        gpr, bounds = _fitted(_banana_ll, 2, 300)
        n = 400
    d = len(bounds)
    logZq, mq, Cq = _quadrature(gpr, bounds, n)
    sd = np.sqrt(np.diag(Cq))
    for seed in (1, 2, 3):
        r = _run(gpr, bounds, seed, nlive=500, num_repeats=5 * d, nprior=5000)
        assert abs(r.logZ - logZq) < 4 * r.logZ_err, (seed, r.logZ, logZq, r.logZ_err)
        m = r.w @ r.X
        C = (r.X - m).T @ ((r.X - m) * r.w[:, None])
        assert np.all(np.abs(m - mq) < 0.1 * sd), (seed, m, mq, sd)
        assert np.all(np.abs(C - Cq) <= 0.2 * np.outer(sd, sd)), (seed, C, Cq)


@pytest.mark.timeout(900)
def test_multi_add_with_the_nested_sampler_matches_the_oracle():
    from gpry_amd.gp_acquisition import NORA
    d, N, npts = 16, 1024, 4
    bounds, X, y = _training(_gauss_ll(d, s=1.5), d, N, 3)
    theta = np.log([4.0] + [0.3] * d)
    gpr = make_gpr(bounds, orc.MATERN52, theta=theta)
    gpr.append_to_data(X, y, fit_gpr=False)
    ref = orc.OracleGPR(bounds, kernel_id=orc.MATERN52)
    ref.theta = theta.copy()
    ref.fitted = True
    ref.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    acq = NORA(bounds, sampler="nested", verbose=0, devices=[0], nlive_max=200, shortlist_size=32)
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(4))
    info = acq.stats["sampler_info"]
    assert info["ncalls"] > 0 and info["generations"] > 0 and info["device_s"] > 0 and np.isfinite(info["logZ"])
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert len(Xs) == info["rows"] and abs(np.sum(ws) - 1.0) < 1e-12
    np.testing.assert_array_equal(ys[:300], _one_point(gpr, Xs[:300]))
    Xo, yo, ao, so, _ = oracle_given(ref, Xs, ys, None, npts, zeta=acq.acq_func.zeta)
    np.testing.assert_array_equal(Xp, Xo)
    np.testing.assert_allclose(yp, yo, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(ap, ao, rtol=1e-7, atol=1e-7)
