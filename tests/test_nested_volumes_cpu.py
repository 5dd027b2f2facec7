"""Per-cluster prior volumes and local evidences in the nested sampler (gpry_amd/nested.py:
run_nested(clustering=True, cluster_volumes=True)) without a device: the numpy stand-in of gpry_ns_generation_volumes
(tests/tools/ns_volumes.py); the calls of the runs without volumes; a one-cluster run against clustering without
volumes; the bookkeeping identities and the modes' evidences on two-Gaussian mixtures; the small mode's mass with and
without volumes; a cluster emptied inside one batch; and the option's way through nested_settings, mc_sample_from_gp
and NORA."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_host_logic_cpu import _golden_model
from test_nested_cpu import NestedFakeGPR
from test_nested_cluster_cpu import _mixture

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_cluster  # noqa: E402
import ns_volumes  # noqa: E402


def _small_mode_mixture(f, d=2, sigma=0.3):
    """Normalised isotropic mixture: weight f at x_0 = -2, 1 - f at x_0 = +2, both of width sigma; on the box [-5, 5]^d
    the evidence is -d log 10."""
    mus = np.zeros((2, d))
    mus[0, 0], mus[1, 0] = -2.0, 2.0
    lw = np.log([f, 1.0 - f]) - d * np.log(sigma) - 0.5 * d * np.log(2 * np.pi)

    def loglike(X):
        X = np.atleast_2d(X)
        comp = [lw[q] - 0.5 * np.sum((X - mus[q]) ** 2, axis=1) / sigma ** 2 for q in range(2)]
        return np.logaddexp(comp[0], comp[1])

    return loglike, np.array([[-5.0, 5.0]] * d), -d * np.log(10.0)


class _Calls:
    """Every call a run makes on a device: (name, positional count, keyword names)."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def call(*a, **kw):
            self.calls.append((name, len(a), tuple(sorted(kw))))
            return fn(*a, **kw)
        return call


def test_runs_without_volumes_make_the_calls_of_before():
    from gpry_amd.nested import run_nested
    loglike, bounds, _, _ = _mixture(2)
    kw = dict(nlive=60, num_repeats=6, nprior=600)
    a = _Calls(ns_volumes.VolumesNumpyDevice(loglike))
    ra = run_nested(a, bounds, 3, clustering=True, cluster_volumes=False, **kw)
    b = _Calls(ns_cluster.ClusteredNumpyDevice(loglike))
    rb = run_nested(b, bounds, 3, clustering=True, **kw)
    assert a.calls == b.calls
    assert a.calls[0] == ("ns_prior", 4, ())
    assert a.calls[1:] == [("ns_knn", 4, ()), ("ns_generation", 10, ("labels",))] * ra.ngen
    np.testing.assert_array_equal(ra.X, rb.X)
    np.testing.assert_array_equal(ra.w, rb.w)
    assert ra.cluster is None and ra.cluster_logZ is None and ra.cluster_parent is None
    c = _Calls(ns_volumes.VolumesNumpyDevice(loglike))
    rc = run_nested(c, bounds, 3, cluster_volumes=False, **kw)
    assert c.calls == [("ns_prior", 4, ())] + [("ns_generation", 10, ())] * rc.ngen
    assert rc.n_clusters is None and rc.cluster is None


def _gauss(d):
    rng = np.random.default_rng(7 + d)
    A = rng.normal(size=(d, d))
    C = 0.05 * (A @ A.T / d + np.eye(d))
    Ci = np.linalg.inv(C)
    mu = rng.uniform(-0.5, 0.5, d)

    def loglike(X):
        Z = np.atleast_2d(X) - mu
        return -0.5 * np.einsum("ni,ij,nj->n", Z, Ci, Z)
    return loglike


@pytest.mark.parametrize("d", [3, 5])
def test_one_cluster_run_equals_clustering_without_volumes(d):
    from gpry_amd.nested import run_nested
    ll, bounds = _gauss(d), np.array([[-3.0, 3.0]] * d)
    kw = dict(nlive=25 * d, num_repeats=2 * d, nprior=250 * d, clustering=True)
    a = run_nested(ns_volumes.VolumesNumpyDevice(ll), bounds, 11, **kw)
    dev = ns_volumes.VolumesNumpyDevice(ll)
    b = run_nested(dev, bounds, 11, cluster_volumes=True, **kw)
    assert np.all(b.n_clusters == 1) and np.array_equal(a.n_clusters, b.n_clusters)
    assert len(dev.volume_calls) == b.ngen
    np.testing.assert_array_equal(b.X, a.X)
    np.testing.assert_array_equal(b.y, a.y)
    assert (b.ncalls, b.ngen) == (a.ncalls, a.ngen)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-12, atol=0)
    assert abs(b.logZ - a.logZ) <= 1e-12 * abs(a.logZ)
    assert b.cluster_parent.tolist() == [-1] and not b.cluster.any()
    assert abs(b.cluster_logZ[0] - b.logZ) <= 1e-12 * abs(b.logZ)


def _mode_logZ(r):
    """Evidence of the modes at x_0 < 0 and x_0 > 0: the subtree of each mode (every non-root cluster goes whole to the
    side that holds most of its weight: a chain may still cross to the other mode while L* is low) plus the root's rows
    on that side."""
    side = r.X[:, 0] < 0
    left = (r.cluster == 0) & side
    for q in range(1, len(r.cluster_parent)):
        rows = r.cluster == q
        if np.sum(r.w[rows & side]) > 0.5 * np.sum(r.w[rows]):
            left |= rows
    with np.errstate(divide="ignore"):
        return r.logZ + np.log(np.sum(r.w[left])), r.logZ + np.log(np.sum(r.w[~left]))


def _check_bookkeeping(r, nlive):
    from gpry_amd.nested import _logsumexp
    par = r.cluster_parent
    ids = np.arange(len(par))
    assert par[0] == -1 and np.all((par[1:] >= 0) & (par[1:] < ids[1:]))
    assert abs(_logsumexp(r.cluster_logZ) - r.logZ) <= 1e-12 * max(1.0, abs(r.logZ))
    assert r.cluster.shape == r.y.shape and np.all((r.cluster >= 0) & (r.cluster < len(par)))
    with np.errstate(divide="ignore"):
        lw = np.log(r.w) + r.logZ
    for q in ids:
        rows = r.cluster == q
        if rows.any():
            assert abs(_logsumexp(lw[rows]) - r.cluster_logZ[q]) <= 1e-9 * max(1.0, abs(r.logZ)), q
    # a row dies in a cluster only while it is open: all of a split cluster's rows come before any of its children's
    pos = np.arange(len(r.cluster))
    for q in ids[1:]:
        rq, rp = r.cluster == q, r.cluster == par[q]
        if rq.any() and rp.any():
            assert pos[rp].max() < pos[rq].min(), (par[q], q)
    # the final live points sit in leaves
    leaves = set(ids.tolist()) - set(par.tolist())
    assert set(r.cluster[-nlive:].tolist()) <= leaves


# a mode's evidence (its subtree plus the root's rows on its side) against the truth, in units of the run's logZ_err:
# over seeds 1 .. 10 of these three cases the largest pull was 3.8 (the 0.7 mode in d = 4), RMS 0.9 - 2.0
MODE_ERR = 5.0


@pytest.mark.parametrize("case", ["0.3/0.7, d=2", "0.3/0.7, d=4", "0.12/0.88, d=2"])
def test_bookkeeping_and_mode_evidences_on_mixtures(case):
    from gpry_amd.nested import run_nested
    if case.startswith("0.3"):
        d = int(case[-1])
        loglike, bounds, logZ_true, ws = _mixture(d)
    else:
        d = 2
        loglike, bounds, logZ_true = _small_mode_mixture(0.12)
        ws = np.array([0.12, 0.88])
    for seed in (1, 2):
        nlive = 100 * d
        r = run_nested(ns_volumes.VolumesNumpyDevice(loglike), bounds, seed, nlive=nlive, num_repeats=5 * d,
                       nprior=10 * nlive, clustering=True, cluster_volumes=True)
        _check_bookkeeping(r, nlive)
        assert len(r.cluster_parent) >= 3 and r.n_clusters.max() >= 2
        assert abs(r.logZ - logZ_true) < 4 * r.logZ_err, (seed, r.logZ, logZ_true, r.logZ_err)
        for got, w in zip(_mode_logZ(r), ws):
            assert abs(got - (logZ_true + np.log(w))) < MODE_ERR * r.logZ_err, (seed, got, w)


# ---- a cluster emptied inside one batch -----------------------------------------------------------------------------
def _two_levels(X):
    """A mode at (2.5, 0) with peak 0 and one at (-2, 0) with peak -40, both of width 0.3."""
    X = np.atleast_2d(X)
    a = -np.sum((X - [2.5, 0.0]) ** 2, axis=1) / 0.18
    b = -40.0 - np.sum((X - [-2.0, 0.0]) ** 2, axis=1) / 0.18
    return np.maximum(a, b)


class _GivenStart(ns_volumes.VolumesNumpyDevice):
    """The prior draw replaced by a given live set."""

    def __init__(self, loglike, X0):
        super().__init__(loglike)
        self.X0 = X0

    def ns_prior(self, lo, hi, seed, n):
        assert n == len(self.X0)
        return self.X0.copy(), np.asarray(self.loglike(self.X0), dtype=float), 0.0


def test_a_cluster_emptied_in_one_batch_is_closed():
    from gpry_amd.nested import run_nested
    rng = np.random.default_rng(0)

    def disc(c, r):
        a = rng.uniform(0, 2 * np.pi, len(r))
        return np.asarray(c) + np.stack([r * np.cos(a), r * np.sin(a)], axis=1)

    # 30 points on a ring around the low mode (the first batch), 8 inside it, 22 at the top of the high mode: after the
    # first kill the low mode's 8 survivors form the first cluster (smallest index), and all its points, old and new,
    # lie below the high mode's, so the second batch of 30 takes every one of them
    X0 = np.concatenate([disc([-2.0, 0.0], rng.uniform(0.30, 0.35, 30)), disc([-2.0, 0.0], rng.uniform(0.0, 0.25, 8)),
                         disc([2.5, 0.0], rng.uniform(0.0, 0.3, 22))])
    dev = _GivenStart(_two_levels, X0)
    r = run_nested(dev, np.array([[-5.0, 5.0]] * 2), 4, nlive=60, num_repeats=4, batch=30, clustering=True,
                   cluster_volumes=True, max_ncalls=40000)
    _check_bookkeeping(r, 60)
    first = dev.volume_calls[0]
    assert first["n_clusters"] == 2 and list(first["counts"]) == [8, 22]
    assert r.cluster_parent[:3].tolist() == [-1, 0, 0] and r.ngen >= 3
    # cluster 1 holds its 8 survivors and the points of the chains that drew it in generation 0, all dead by the end
    # of the second batch (the prior's 60 rows and two batches of 30); no later generation offers it to a chain
    rows = np.flatnonzero(r.cluster == 1)
    assert len(rows) == 8 + int(np.sum(first["drawn"] == 0)) and rows.max() < 90
    assert np.all(r.X[rows, 0] < 0) and not np.any(r.X[90:, 0] < 0)
    for call in dev.volume_calls[1:]:
        assert call["counts"].sum() == 30
    assert 1 not in r.cluster[r.n_dead:].tolist() and np.isfinite(r.cluster_logZ[1])


# ---- the small mode's mass with and without volumes -----------------------------------------------------------------
def test_small_mode_mass_with_and_without_volumes():
    """profiles/nested_volumes.md: weight 0.15 at nlive = 50 (num_repeats 10, nprior 10 nlive), 24 seeds from 1000: with
    volumes the mode was never lost (mass below a third of the truth) against 2 of 24 without, at an RMS error of 0.057
    against 0.060 -- the spread itself is not smaller.  These are the first 16 of those seeds; the bounds keep a margin
    of about 1.5 x on the measured RMS."""
    from gpry_amd.nested import run_nested
    f = 0.15
    loglike, bounds, _ = _small_mode_mixture(f)
    mass = {}
    for vol in (False, True):
        mass[vol] = np.array([np.sum(r.w[r.X[:, 0] < 0]) for r in (
            run_nested(ns_volumes.VolumesNumpyDevice(loglike), bounds, 1000 + s, nlive=50, num_repeats=10, nprior=500,
                       clustering=True, cluster_volumes=vol) for s in range(16))])
    rms = {v: float(np.sqrt(np.mean((m - f) ** 2))) for v, m in mass.items()}
    assert np.all(mass[True] > f / 3), mass[True]
    assert rms[True] < 0.085 and rms[True] < rms[False] + 0.02, rms


# ---- the option's way through the package -----------------------------------------------------------------------------
def test_nested_settings_cluster_volumes_key():
    from gpry_amd.mc import nested_settings
    assert "cluster_volumes" not in nested_settings(3)
    assert "cluster_volumes" not in nested_settings(3, {"clustering": True})
    assert nested_settings(3, {"clustering": True, "cluster_volumes": True})["cluster_volumes"] is True
    assert nested_settings(3, {"clustering": True, "cluster_volumes": False})["cluster_volumes"] is False
    assert nested_settings(3, {"cluster_volumes": False})["cluster_volumes"] is False
    for opts in ({"cluster_volumes": True}, {"clustering": False, "cluster_volumes": True}):
        with pytest.raises(ValueError, match="cluster_volumes"):
            nested_settings(3, opts)


def test_volumes_without_clustering_are_refused():
    from gpry_amd.gp_acquisition import NORA
    from gpry_amd.nested import run_nested
    loglike, bounds, _, _ = _mixture(2)
    with pytest.raises(ValueError, match="cluster_volumes"):
        run_nested(ns_volumes.VolumesNumpyDevice(loglike), bounds, 1, nlive=20, num_repeats=2, cluster_volumes=True)
    with pytest.raises(ValueError, match="nested_cluster_volumes"):
        NORA(bounds, sampler="nested", verbose=0, nested_cluster_volumes=True)


def _fake_gpr():
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = NestedFakeGPR(m)
    gpr.device.ns = ns_volumes.VolumesNumpyDevice(lambda X: m.predict(X))
    gpr.device.ns_prior, gpr.device.ns_generation = gpr.device.ns.ns_prior, gpr.device.ns.ns_generation
    gpr.device.ns_knn = gpr.device.ns.ns_knn
    return gpr, bounds


def _spy(monkeypatch):
    from gpry_amd import nested
    seen, real = [], nested.run_nested

    def spy(dev, b, seed, nlive, num_repeats, **kw):
        seen.append(kw)
        return real(dev, b, seed, nlive, num_repeats, **kw)

    monkeypatch.setattr(nested, "run_nested", spy)
    return seen


def test_mc_sample_from_gp_passes_the_volumes_flag(monkeypatch):
    from gpry_amd import mc
    seen = _spy(monkeypatch)
    gpr, bounds = _fake_gpr()
    gpr.minus_inf_value = -np.inf
    gpr.trust_bounds = None
    gpr.bounds = np.asarray(bounds, dtype=float)
    gpr._ensure_factor = gpr._push_affine = lambda: None
    opts = {"nlive": "5d", "num_repeats": 2, "precision_criterion": 0.1, "clustering": True}
    mc.mc_sample_from_gp(gpr, sampler_options=opts, seed=4)
    assert "cluster_volumes" not in seen[-1] and mc.mc_sample_from_gp.last_result.cluster_logZ is None
    mc.mc_sample_from_gp(gpr, sampler_options={**opts, "cluster_volumes": True}, seed=4)
    assert seen[-1]["clustering"] is True and seen[-1]["cluster_volumes"] is True
    res = mc.mc_sample_from_gp.last_result
    assert res.cluster_logZ is not None and len(res.cluster) == len(res.y)


def test_nora_passes_the_volumes_flag_and_reports_local_evidences(monkeypatch):
    from gpry_amd.gp_acquisition import NORA
    seen = _spy(monkeypatch)
    gpr, bounds = _fake_gpr()
    kw = dict(sampler="nested", verbose=0, nlive_max=30, num_repeats=4, nprior_per_nlive=3, nested_clustering=True)
    off = NORA(bounds, **kw)
    off.do_MC_sample(gpr, None, rng=np.random.default_rng(5))
    assert "cluster_volumes" not in seen[-1]
    assert "cluster_logZ" not in off.stats["sampler_info"] and "cluster_parent" not in off.stats["sampler_info"]
    on = NORA(bounds, nested_cluster_volumes=True, **kw)
    on.do_MC_sample(gpr, None, rng=np.random.default_rng(5))
    assert seen[-1]["clustering"] is True and seen[-1]["cluster_volumes"] is True
    info = on.stats["sampler_info"]
    assert set(info["cluster_logZ"]) == set(info["cluster_parent"]) and info["cluster_parent"][0] == -1
    from gpry_amd.nested import _logsumexp
    assert abs(_logsumexp(list(info["cluster_logZ"].values())) - info["logZ"]) <= 1e-12 * max(1.0, abs(info["logZ"]))
    assert on.update_NS_precision(gpr) == off.update_NS_precision(gpr)
