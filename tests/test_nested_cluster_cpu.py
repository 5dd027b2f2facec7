"""Clustering of the nested sampler's live set (gpry_amd/nested.py: knn_clusters, run_nested(clustering=True)) without a
device: the numpy neighbour table of tests/tools/ns_cluster.py, the clustering rule on seeded synthetic live sets, a run
on an analytic two-Gaussian mixture with the numpy stand-in of the clustered generation, and the flag's way through NORA
and mc_sample_from_gp."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from test_host_logic_cpu import _golden_model
from test_nested_cpu import NestedFakeGPR

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_cluster  # noqa: E402
import ns_philox  # noqa: E402


def _blob(rng, n, d, c, s):
    """n points of a Gaussian of scale s around c with a random orientation and axis variances in [0.25, 1] s^2."""
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    L = Q * np.sqrt(rng.uniform(0.25, 1.0, d))
    return c + s * rng.normal(size=(n, d)) @ L.T


def _centres(rng, d, m, sep):
    """m centres at mutual distances >= sep around 0.5: the vertices of an equilateral triangle in a random plane."""
    Q, _ = np.linalg.qr(rng.normal(size=(d, 2)))
    ang = 2 * np.pi * np.arange(m) / 3
    r = sep / np.sqrt(3.0)
    return 0.5 + r * (np.outer(np.cos(ang), Q[:, 0]) + np.outer(np.sin(ang), Q[:, 1]))


def _clusters(X, d, k_max=10):
    from gpry_amd.nested import knn_clusters
    nbr = ns_cluster.knn_table(X, np.zeros(d), np.ones(d), k_max)
    return knn_clusters(nbr, d, k_max)


def _case(d, seed, what):
    rng = np.random.default_rng(seed)
    n, s = 25 * d, 0.01
    c = _centres(rng, d, 3, 20 * s)
    if what == "one":
        return _blob(rng, n, d, c[0], s), 1
    if what == "small":
        return np.concatenate([_blob(rng, n, d, c[0], s), _blob(rng, d, d, c[1], s)]), 1
    m = {"two": 2, "three": 3}[what]
    return np.concatenate([_blob(rng, n, d, c[q], s) for q in range(m)]), m


@pytest.mark.parametrize("d", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("what", ["one", "two", "three", "small"])
def test_clusters_of_synthetic_live_sets(d, what):
    hits = []
    for seed in range(20):
        X, m = _case(d, seed, what)
        labels, nc = _clusters(X, d)
        hits.append(nc == m)
        if nc == m and m > 1:
            # the clusters are the blobs, numbered by their smallest member
            n = len(X) // m
            np.testing.assert_array_equal(labels, np.repeat(np.arange(m), n))
    # In two dimensions a blob of 25 d = 50 points is sparse enough that its 2- and 3-neighbour graphs now and then
    # split off the same group of tail points (a stable partition of clusters >= d + 1), which the rule keeps: measured
    # 1 to 3 of these 20 seeds per case (profiles/nested_clusters.md).  From d = 4 on, every seed.
    need = 17 if d == 2 else 20
    assert sum(hits) >= need, hits


def test_unstable_or_single_component_is_one_cluster():
    from gpry_amd.nested import knn_clusters
    rng = np.random.default_rng(0)
    d = 3
    X, _ = _case(d, 1, "two")
    nbr = ns_cluster.knn_table(X, np.zeros(d), np.ones(d), 10)
    assert knn_clusters(nbr, d, 10)[1] == 2
    # k_max = 2 leaves no k >= 3 to confirm the partition; min_size above a blob's size rejects it
    assert knn_clusters(nbr, d, 2)[1] == 1
    assert knn_clusters(nbr, d, 10, min_size=len(X) // 2 + 1)[1] == 1
    labels, nc = knn_clusters(ns_cluster.knn_table(rng.uniform(size=(200, d)), np.zeros(d), np.ones(d), 10), d, 10)
    assert nc == 1 and labels.dtype == np.int32 and not labels.any()


def _reference_table(X, lo, hi, k):
    """Row by row with Python sorting: the definition of the table."""
    U = (np.asarray(X, float) - lo) / (hi - lo)
    out = []
    for i in range(len(U)):
        d2 = []
        for j in range(len(U)):
            s = 0.0
            for c in range(U.shape[1]):
                s = s + (U[i, c] - U[j, c]) * (U[i, c] - U[j, c])
            d2.append((s, j))
        out.append([j for s, j in sorted(d2) if j != i][:k])
    return np.array(out)


@pytest.mark.parametrize("d", [1, 3])
def test_numpy_neighbour_table(d):
    rng = np.random.default_rng(d)
    lo, hi = -2.0 * np.ones(d), 3.0 * np.ones(d)
    X = rng.uniform(-2, 3, (40, d))
    X[10:15] = X[3]                      # duplicated points: distance 0, ordered by index
    X[20] = X[21]
    nbr = ns_cluster.knn_table(X, lo, hi, 12)
    np.testing.assert_array_equal(nbr, _reference_table(X, lo, hi, 12))
    assert not np.any(nbr == np.arange(40)[:, None])
    assert list(nbr[3, :5]) == [10, 11, 12, 13, 14] and list(nbr[10, :5]) == [3, 11, 12, 13, 14]
    assert nbr[20, 0] == 21 and nbr[21, 0] == 20
    U = (X - lo) / (hi - lo)
    for i in range(40):
        dist = np.sum((U[nbr[i]] - U[i]) ** 2, axis=1)
        assert np.all(np.diff(dist) >= 0)
    np.testing.assert_array_equal(ns_cluster.knn_table(X, lo, hi, 12, rows=np.array([5, 20])), nbr[[5, 20]])


# ---- a run on a two-Gaussian mixture --------------------------------------------------------------------------------
def _mixture(d):
    """Unequal weights 0.3 / 0.7, modes at x_0 = -2 and +2, differently oriented covariances; normalised, so that with the
    box [-5, 5]^d the evidence against the uniform prior is -d log 10 (the mass outside the box is below 1e-9)."""
    rng = np.random.default_rng(100 + d)
    mus = np.zeros((2, d))
    mus[0, 0], mus[1, 0] = -2.0, 2.0
    covs = []
    for q in range(2):
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        covs.append(Q @ np.diag(rng.uniform(0.04, 0.16, d)) @ Q.T)
    ws = np.array([0.3, 0.7])
    Ci = [np.linalg.inv(C) for C in covs]
    lnorm = [-0.5 * np.linalg.slogdet(2 * np.pi * C)[1] for C in covs]

    def loglike(X):
        X = np.atleast_2d(X)
        comp = [np.log(ws[q]) + lnorm[q] - 0.5 * np.einsum("ni,ij,nj->n", X - mus[q], Ci[q], X - mus[q]) for q in range(2)]
        return np.logaddexp(comp[0], comp[1])

    return loglike, np.array([[-5.0, 5.0]] * d), -d * np.log(10.0), ws


@pytest.mark.parametrize("d", [2, 5])
def test_clustered_run_on_a_two_gaussian_mixture(d):
    from gpry_amd.nested import run_nested
    loglike, bounds, logZ, ws = _mixture(d)
    # Once the modes separate, a new point joins the mode of its (uniformly drawn) start, so the modes' live counts
    # drift: the mass split has a spread of order 1 / sqrt(nlive) times that drift (PolyChord's per-cluster volumes
    # remove it; they are not done here).  nlive = 300 d keeps it well inside 0.05.
    for seed in (1, 2):
        dev = ns_cluster.ClusteredNumpyDevice(loglike)
        r = run_nested(dev, bounds, seed, nlive=300 * d, num_repeats=5 * d, precision_criterion=0.01, nprior=3000 * d,
                       clustering=True)
        assert abs(r.logZ - logZ) < 4 * r.logZ_err, (seed, r.logZ, logZ, r.logZ_err)
        frac = np.sum(r.w[r.X[:, 0] < 0])
        assert abs(frac - ws[0]) < 0.05, (seed, frac)
        assert r.n_clusters is not None and len(r.n_clusters) == r.ngen and r.n_clusters.max() >= 2
        assert len(dev.knn_calls) == r.ngen and dev.clustered_calls == r.ngen


class _Recorder:
    """The two unclustered calls of a numpy device, and nothing else."""

    def __init__(self, loglike):
        self.inner, self.calls = ns_philox.NumpyNestedDevice(loglike), []

    def ns_prior(self, *a):
        self.calls.append(("ns_prior", len(a)))
        return self.inner.ns_prior(*a)

    def ns_generation(self, *a, **kw):
        self.calls.append(("ns_generation", len(a), tuple(kw)))
        return self.inner.ns_generation(*a, **kw)


def test_clustering_off_makes_the_calls_of_before():
    from gpry_amd.nested import run_nested
    loglike, bounds, _, _ = _mixture(2)
    dev = _Recorder(loglike)
    r = run_nested(dev, bounds, 3, nlive=40, num_repeats=6, nprior=120)
    assert r.n_clusters is None
    assert dev.calls[0] == ("ns_prior", 4)
    assert dev.calls[1:] == [("ns_generation", 10, ())] * r.ngen
    # the clustered stand-in with one cluster everywhere gives the unclustered run's bits
    a = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, 3, nlive=40, num_repeats=6, nprior=120)
    np.testing.assert_array_equal(a.X, r.X)


def test_nested_settings_clustering_key():
    from gpry_amd.mc import nested_settings
    assert "clustering" not in nested_settings(3)
    assert nested_settings(3, {"clustering": True})["clustering"] is True
    assert nested_settings(3, {"clustering": False})["clustering"] is False
    with pytest.warns(UserWarning, match="do_clustering") as w:
        s = nested_settings(2, {"do_clustering": True})
    assert "clustering" not in s and "'clustering'" in str(w[0].message)


def test_mc_sample_from_gp_passes_the_flag(monkeypatch):
    from gpry_amd import mc, nested
    seen = []
    real = nested.run_nested

    def spy(dev, b, seed, nlive, num_repeats, **kw):
        seen.append(kw)
        return real(dev, b, seed, nlive, num_repeats, **kw)

    monkeypatch.setattr(nested, "run_nested", spy)
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = NestedFakeGPR(m)
    gpr.device.ns = ns_cluster.ClusteredNumpyDevice(lambda X: m.predict(X))
    gpr.device.ns_prior, gpr.device.ns_generation = gpr.device.ns.ns_prior, gpr.device.ns.ns_generation
    gpr.device.ns_knn = gpr.device.ns.ns_knn
    gpr.minus_inf_value = -np.inf
    gpr.trust_bounds = None
    gpr.bounds = np.asarray(bounds, dtype=float)
    gpr._ensure_factor = gpr._push_affine = lambda: None
    opts = {"nlive": "5d", "num_repeats": 2, "precision_criterion": 0.1}
    mc.mc_sample_from_gp(gpr, sampler_options=opts, seed=4)
    mc.mc_sample_from_gp(gpr, sampler_options={**opts, "clustering": True}, seed=4)
    assert "clustering" not in seen[0] and seen[1]["clustering"] is True
    assert mc.mc_sample_from_gp.last_result.n_clusters is not None
    assert len(mc.mc_sample_from_gp.last_result.n_clusters) == mc.mc_sample_from_gp.last_result.ngen


def test_nora_passes_the_flag_and_reports_clusters(monkeypatch):
    from gpry_amd import nested
    from gpry_amd.gp_acquisition import NORA
    seen = []
    real = nested.run_nested

    def spy(dev, b, seed, nlive, num_repeats, **kw):
        seen.append(kw)
        return real(dev, b, seed, nlive, num_repeats, **kw)

    monkeypatch.setattr(nested, "run_nested", spy)
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = NestedFakeGPR(m)
    gpr.device.ns = ns_cluster.ClusteredNumpyDevice(lambda X: m.predict(X))
    gpr.device.ns_prior, gpr.device.ns_generation = gpr.device.ns.ns_prior, gpr.device.ns.ns_generation
    gpr.device.ns_knn = gpr.device.ns.ns_knn
    kw = dict(sampler="nested", verbose=0, nlive_max=30, num_repeats=4, nprior_per_nlive=3)
    off = NORA(bounds, **kw)
    off.do_MC_sample(gpr, None, rng=np.random.default_rng(5))
    assert "clustering" not in seen[-1] and "clusters" not in off.stats["sampler_info"]
    on = NORA(bounds, nested_clustering=True, **kw)
    on.do_MC_sample(gpr, None, rng=np.random.default_rng(5))
    assert seen[-1]["clustering"] is True
    assert on.stats["sampler_info"]["clusters"] >= 1
    assert set(on.update_NS_precision(gpr)) == set(off.update_NS_precision(gpr))


def test_cluster_k_max_is_checked():
    from gpry_amd.nested import run_nested
    loglike, bounds, _, _ = _mixture(2)
    with pytest.raises(ValueError, match="cluster_k_max"):
        run_nested(ns_cluster.ClusteredNumpyDevice(loglike), bounds, 1, nlive=20, num_repeats=2, clustering=True,
                   cluster_k_max=40)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = run_nested(ns_cluster.ClusteredNumpyDevice(loglike), bounds, 1, nlive=20, num_repeats=2, clustering=True,
                       cluster_k_max=3, max_ncalls=500)
    assert r.ngen >= 1
