"""Phantom points of the nested sampler (gpry_amd/nested.py: ``merged_weights``, ``run_nested(phantom_thin=)``) driven by
the numpy stand-in of tests/tools/ns_phantoms.py, and their way through ``nested_settings`` / ``mc_sample_from_gp`` and
NORA: the merged live counts against a brute-force count; the run with phantoms is the run without plus rows; the merged
evidence and mean of an analytic Gaussian within the bounds of test_evidence_of_an_analytic_gaussian; plateaus; the
refusals; the phantom rows and their y reach the given-y sweep."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT
from test_given_y_cpu import oracle_given
from test_host_logic_cpu import _golden_model
from test_nested_cpu import NestedFakeGPR, _gauss

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_phantoms  # noqa: E402


# ---- merged_weights ---------------------------------------------------------------------------------------------------
def _hand_built():
    """9 prior points (two outside, one tie) and three generations; generation 1's threshold equals a point's L, and a
    point of generation 1 sits on that threshold (a chain that stayed on a plateau)."""
    inf = np.inf
    L = np.array([-inf, -3.0, -inf, -2.0, -2.0, -1.0, 0.5, -0.5, 1.5,         # prior
                  -1.5, -0.2, 0.3, -0.9,                                     # generation 0, thr -2.0
                  -0.5, 0.1, 0.1, 1.0,                                       # generation 1, thr -0.5 (tie: rows 7, 13)
                  0.4, 2.0, 0.9])                                            # generation 2, thr 0.3
    born = np.array([-1] * 9 + [0] * 4 + [1] * 4 + [2] * 3)
    thr = np.array([-2.0, -0.5, 0.3])
    return L, born, thr


def _weights_from_counts(L, born, cnt, L_end):
    """The definition, one point at a time, from given live counts."""
    order = sorted(range(len(L)), key=lambda i: (L[i], born[i], i))
    logw = np.full(len(L), -np.inf)
    logX = 0.0
    final = [i for i in order if L[i] > L_end]
    for i in order:
        if L[i] > L_end:
            break
        if np.isfinite(L[i]):
            logw[i] = L[i] + logX - np.log(cnt[i] + 1.0)
        logX += np.log(cnt[i] / (cnt[i] + 1.0))
    for i in final:
        logw[i] = L[i] + logX - np.log(len(final))
    return logw


def test_merged_weights_against_a_brute_force_live_count():
    from gpry_amd.nested import merged_weights
    L, born, thr = _hand_built()
    cnt = ns_phantoms.live_counts_brute(L, born, thr)
    assert np.all(cnt >= 1)
    # the count by hand at a few places: the two outside points die first among 9; the point on the threshold of its own
    # generation (row 13) dies after row 7 with the whole of generation 1 present
    assert cnt[0] == 9 and cnt[2] == 8 and cnt[1] == 7
    assert cnt[7] == 9 - 6 + 4 - 2 and cnt[13] == cnt[7] - 1 + 4
    for L_end in (None, 0.3, -0.5, -np.inf):
        logw, logZ = merged_weights(L, born, thr, L_end=L_end)
        want = _weights_from_counts(L, born, cnt, thr[-1] if L_end is None else L_end)
        np.testing.assert_allclose(logw, want, rtol=1e-13, atol=1e-13)
        assert logw[0] == logw[2] == -np.inf
        m = np.max(want)
        assert abs(logZ - (m + np.log(np.sum(np.exp(want - m))))) < 1e-13
    # a random set with many ties and thresholds that repeat
    rng = np.random.default_rng(0)
    thr = np.array([-1.0, -1.0, 0.0, 0.5, 0.5])
    born = np.concatenate([np.full(30, -1), rng.integers(0, 5, 60)])
    L = np.round(rng.normal(size=90), 1)
    gen = born >= 0
    L[gen] = np.maximum(L[gen], thr[born[gen]])           # at or above the threshold of its generation
    L[rng.choice(30, 4, replace=False)] = -np.inf
    cnt = ns_phantoms.live_counts_brute(L, born, thr)
    assert np.all(cnt >= 1)
    logw, _ = merged_weights(L, born, thr)
    np.testing.assert_allclose(logw, _weights_from_counts(L, born, cnt, thr[-1]), rtol=1e-13, atol=1e-13)


def test_merged_weights_refuses_inconsistent_input():
    from gpry_amd.nested import merged_weights
    with pytest.raises(ValueError, match="non-decreasing"):
        merged_weights([0.0, 1.0], [-1, 0], [0.5, 0.2])
    with pytest.raises(ValueError, match="born"):
        merged_weights([0.0, 1.0], [-1, 1], [0.5])


# ---- the run ----------------------------------------------------------------------------------------------------------
def _ess(w):
    return 1.0 / np.sum(w ** 2)


@pytest.mark.parametrize("clustering", [False, True])
def test_the_run_with_phantoms_is_the_run_without_plus_rows(clustering):
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(3)
    kw = dict(nlive=40, num_repeats=7, nprior=160, clustering=clustering)
    a = run_nested(ns_phantoms.PhantomNumpyDevice(loglike), bounds, 5, **kw)
    assert a.phantom is None and a.logZ_merged is None and a.n_phantom is None
    for thin in (1, 3):
        dev = ns_phantoms.PhantomNumpyDevice(loglike)
        b = run_nested(dev, bounds, 5, phantom_thin=thin, **kw)
        n = len(a.y)
        n_ph = (7 - 1) // thin
        assert b.n_phantom == b.ngen * 20 * n_ph == int(b.phantom.sum()) and len(b.y) == n + b.n_phantom
        assert not b.phantom[:n].any() and b.phantom[n:].all()
        np.testing.assert_array_equal(b.X[:n], a.X)
        np.testing.assert_array_equal(b.y[:n], a.y)
        for f in ("logZ", "logZ_err", "ncalls", "ngen", "n_dead"):
            assert getattr(b, f) == getattr(a, f), f
        np.testing.assert_array_equal(b.dead_L, a.dead_L)
        np.testing.assert_array_equal(b.dead_logX, a.dead_logX)
        if clustering:
            np.testing.assert_array_equal(b.n_clusters, a.n_clusters)
        assert len(b.w) == len(b.y) and np.all(b.w >= 0) and abs(np.sum(b.w) - 1.0) < 1e-12
        assert np.all(np.isfinite(b.y)) and np.isfinite(b.logZ_merged)
        assert np.all((b.X >= bounds[:, 0]) & (b.X <= bounds[:, 1]))
        np.testing.assert_array_equal(b.y[n:], loglike(b.X[n:]))
        # (generation, chain, slot) order, every phantom above the threshold of its generation
        assert [c["n_ph"] for c in dev.phantom_calls] == [n_ph] * b.ngen
        assert all(c["clustered"] == clustering for c in dev.phantom_calls)
        thr = np.repeat([c["lstar"] for c in dev.phantom_calls], 20 * n_ph)
        assert np.all(b.y[n:] > thr)
        assert _ess(b.w) > _ess(a.w)


def test_without_recorded_states_the_weights_are_those_of_the_plain_run():
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(3)
    # a third of the box is outside: those points die first and count in the volumes
    def ll(X):
        y = loglike(X)
        y[X[:, 0] > 2.0] = -np.inf
        return y
    kw = dict(nlive=40, num_repeats=6, nprior=200, batch=10)
    a = run_nested(ns_phantoms.PhantomNumpyDevice(ll), bounds, 7, **kw)
    for thin in (6, 50):
        b = run_nested(ns_phantoms.PhantomNumpyDevice(ll), bounds, 7, phantom_thin=thin, **kw)
        assert b.n_phantom == 0 and len(b.y) == len(a.y) and not b.phantom.any()
        np.testing.assert_allclose(b.w, a.w, rtol=1e-12)
        assert abs(b.logZ_merged - a.logZ) < 1e-12
        np.testing.assert_array_equal(b.X, a.X)


@pytest.mark.parametrize("thin", [1, 2])
@pytest.mark.parametrize("d", [2, 5])
def test_merged_evidence_of_an_analytic_gaussian(d, thin):
    """The settings and bounds of test_evidence_of_an_analytic_gaussian, for the merged evidence and mean."""
    from gpry_amd.nested import run_nested
    loglike, bounds, logZ = _gauss(d)
    for seed in (1, 2):
        r = run_nested(ns_phantoms.PhantomNumpyDevice(loglike), bounds, seed, nlive=25 * d, num_repeats=5 * d,
                       precision_criterion=0.01, nprior=250 * d, phantom_thin=thin)
        print(f"d={d} thin={thin} seed={seed}: logZ {r.logZ:.4f} merged {r.logZ_merged:.4f} true {logZ:.4f} "
              f"err {r.logZ_err:.4f} rows {len(r.y)} ESS {_ess(r.w):.0f}")
        assert r.n_phantom > 0
        assert abs(r.logZ_merged - logZ) < 4 * r.logZ_err, (r.logZ_merged, logZ, r.logZ_err)
        assert np.all(r.w >= 0) and abs(np.sum(r.w) - 1.0) < 1e-12
        m = np.average(r.X, weights=r.w, axis=0)
        assert np.all(np.abs(m - 0.3) < 0.15), m


def test_plateau_likelihood_gives_finite_non_negative_weights():
    """Constant above a level: the thresholds reach the plateau, chains stay on their starts and every new point and
    phantom ties with the threshold of its generation."""
    from gpry_amd.nested import merged_weights, run_nested
    loglike, bounds, _ = _gauss(2)
    level = float(loglike(np.array([[0.3 + 0.6, 0.3]]))[0])

    def ll(X):
        return np.minimum(loglike(X), level)

    r = run_nested(ns_phantoms.PhantomNumpyDevice(ll), bounds, 3, nlive=30, num_repeats=4, nprior=90, phantom_thin=1,
                   precision_criterion=0.05)
    assert np.count_nonzero(r.y == level) > 30 and r.n_phantom > 0
    assert np.all(np.isfinite(r.w)) and np.all(r.w >= 0) and abs(np.sum(r.w) - 1.0) < 1e-12
    assert np.isfinite(r.logZ_merged)
    # the live counts of such a set stay positive without the clamp: ties are broken by generation
    L = np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    born = np.array([-1, -1, -1, 0, 0, 1, 1])
    thr = np.array([1.0, 1.0])
    assert np.all(ns_phantoms.live_counts_brute(L, born, thr) >= 1)
    logw, logZ = merged_weights(L, born, thr)
    assert np.all(np.isfinite(logw)) and np.isfinite(logZ)


# ---- refusals and options ---------------------------------------------------------------------------------------------
def test_refusals():
    from gpry_amd.gp_acquisition import NORA
    from gpry_amd.mc import nested_settings
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(2)
    dev = ns_phantoms.PhantomNumpyDevice(loglike)
    with pytest.raises(ValueError, match="cluster_volumes"):
        run_nested(dev, bounds, 1, nlive=20, num_repeats=3, clustering=True, cluster_volumes=True, phantom_thin=1)
    for thin in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="phantom_thin"):
            run_nested(dev, bounds, 1, nlive=20, num_repeats=3, phantom_thin=thin)
    assert not dev.calls and not dev.phantom_calls
    with pytest.raises(ValueError, match="nested_cluster_volumes"):
        NORA(bounds, sampler="nested", verbose=0, nested_clustering=True, nested_cluster_volumes=True, nested_phantoms=2)
    with pytest.raises(ValueError, match="nested_phantoms"):
        NORA(bounds, sampler="nested", verbose=0, nested_phantoms=-1)
    assert NORA(bounds, sampler="nested", verbose=0).nested_phantoms is None
    assert NORA(bounds, sampler="nested", verbose=0, nested_phantoms=0).nested_phantoms is None
    assert NORA(bounds, sampler="nested", verbose=0, nested_phantoms=3).nested_phantoms == 3
    # the sampler option
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert "phantom_thin" not in nested_settings(3)
        assert "phantom_thin" not in nested_settings(3, {"phantom_thin": None})
        assert nested_settings(3, {"phantom_thin": 2})["phantom_thin"] == 2
    for t in (0, -1, 2.5):
        with pytest.raises(ValueError, match="phantom_thin"):
            nested_settings(3, {"phantom_thin": t})
    with pytest.raises(ValueError, match="cluster_volumes"):
        nested_settings(3, {"phantom_thin": 1, "clustering": True, "cluster_volumes": True})
    with pytest.warns(UserWarning, match="phantoms") as w:
        s = nested_settings(3, {"phantoms": 2})
    assert "phantom_thin" not in s and "phantom_thin" in str(w[0].message)      # (the list of known keys names it)


# ---- mc_sample_from_gp and NORA ---------------------------------------------------------------------------------------
def _fake_gpr(which):
    g, p, bounds, Xc, m = _golden_model(which)
    gpr = NestedFakeGPR(m)
    ns = gpr.device.ns = ns_phantoms.PhantomNumpyDevice(lambda X: m.predict(X))
    gpr.device.ns_prior, gpr.device.ns_generation, gpr.device.ns_knn = ns.ns_prior, ns.ns_generation, ns.ns_knn
    gpr.device.ns_generation_phantoms = ns.ns_generation_phantoms
    return gpr, np.asarray(bounds, dtype=float), m


def test_mc_sample_from_gp_passes_the_option():
    from gpry_amd import mc
    gpr, bounds, m = _fake_gpr("a")
    gpr.minus_inf_value = -np.inf
    gpr.trust_bounds = None
    gpr.bounds = bounds
    gpr._ensure_factor = gpr._push_affine = lambda: None
    opts = {"nlive": "5d", "num_repeats": 4, "precision_criterion": 0.1}
    X0, y0, w0 = mc.mc_sample_from_gp(gpr, sampler_options=opts, seed=4)
    assert mc.mc_sample_from_gp.last_result.phantom is None and not gpr.device.ns.phantom_calls
    X1, y1, w1 = mc.mc_sample_from_gp(gpr, sampler_options={**opts, "phantom_thin": 1}, seed=4)
    res = mc.mc_sample_from_gp.last_result
    assert [c["thin"] for c in gpr.device.ns.phantom_calls] == [1] * res.ngen
    assert res.n_phantom == res.ngen * (5 * len(bounds) // 2) * 3
    assert len(X1) == len(X0) + res.n_phantom and res.n_phantom > 0
    np.testing.assert_array_equal(X1[:len(X0)], X0)
    assert abs(np.sum(w1) - 1.0) < 1e-12 and len(w1) == len(y1) == len(X1)


def test_nora_hands_the_phantom_rows_and_their_y_to_the_given_y_sweep():
    from gpry_amd.gp_acquisition import NORA
    npts = 3
    kw = dict(sampler="nested", verbose=0, nlive_max=30, num_repeats=4, nprior_per_nlive=3)
    gpr0, bounds, m = _fake_gpr("b")
    off = NORA(bounds, **kw)
    off.multi_add(gpr0, n_points=npts, rng=np.random.default_rng(9))
    X0, y0, _, w0 = off.last_MC_sample()
    assert "phantom_rows" not in off.stats["sampler_info"] and not gpr0.device.ns.phantom_calls
    gpr, bounds, m = _fake_gpr("b")
    acq = NORA(bounds, nested_phantoms=1, **kw)
    given, sweep = [], gpr.device.sweep_logexp

    def spy(X, *a, **k):
        given.append((None if X is None else np.array(X), np.array(k["y_given"])))
        return sweep(X, *a, **k)

    gpr.device.sweep_logexp = spy
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(9))
    c = gpr.device.calls[-1]
    assert c["given"] and not c["both"]
    X, y, s, w = acq.last_MC_sample()
    info = acq.stats["sampler_info"]
    assert info["phantom_thin"] == 1 and info["phantom_rows"] == info["generations"] * 15 * 3 > 0
    assert info["rows"] == len(X) == len(X0) + info["phantom_rows"]
    assert np.isfinite(info["logZ_merged"]) and info["logZ"] == off.stats["sampler_info"]["logZ"]
    assert info["ncalls"] == off.stats["sampler_info"]["ncalls"]
    np.testing.assert_array_equal(X[:len(X0)], X0)
    np.testing.assert_array_equal(y[:len(X0)], y0)
    np.testing.assert_allclose(y, m.predict(X), rtol=1e-12)   # (the oracle's batched mean: bits depend on the batch)
    assert w is not None and len(w) == len(X) and abs(np.sum(w) - 1) < 1e-12
    # the sweep ranked the whole pool, phantoms included, with y as given
    Xr, yr, ar, _, _ = oracle_given(m, X, y, None, npts)
    np.testing.assert_array_equal(Xp, Xr)
    np.testing.assert_allclose(ap, ar, rtol=1e-9)
    assert len(given) == 1 and len(given[0][1]) == len(X)
    np.testing.assert_array_equal(given[0][1], y)
    if given[0][0] is not None:
        np.testing.assert_array_equal(given[0][0], X)
