"""Per-cluster volumes in the device nested sampler: gpry_ns_generation_volumes with one cluster is gpry_ns_generation bit
for bit; a chain that drew cluster q is, bit for bit, chain c of gpry_ns_generation on q's survivors with q's matrix;
the drawn clusters are those of the host's restatement (gpry_amd.nested.chain_clusters, which run_nested uses to place
every new point) and follow cum_p; invalid inputs are refused and the context stays usable; a run gives the same bits on
two contexts; on the fitted bimodal surrogate each mode's evidence and mass agree with a quadrature of gpr.predict; and
NORA(nested_cluster_volumes=True).multi_add agrees with the oracle's ranking of the same pool with y given."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import gpry_oracle as orc
from test_given_y_cpu import oracle_given
from test_host_mirror_gpu import make_gpr
from test_nested_cluster_gpu import _bimodal_ll, _fitted_bimodal, _generation_inputs
from test_nested_gpu import _one_point, _quadrature, _run
from test_nested_volumes_cpu import _check_bookkeeping, _mode_logZ

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_volumes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_volumes_generation_with_one_cluster_is_the_unclustered_one():
    from gpry_amd.nested import whitening
    d = 4
    gpr, lo, hi, Xs, ys, lstar = _generation_inputs(d, 3)
    W = whitening((Xs - lo) / (hi - lo))
    a = gpr.device.ns_generation(lo, hi, Xs, ys, lstar, W, 9, 5, 64, 8)
    b = gpr.device.ns_generation(lo, hi, Xs, ys, lstar, W[None], 9, 5, 64, 8, labels=np.zeros(len(Xs), np.int32),
                                 cum_p=[1.0])
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)


def _three_clusters(d, Xs, seed=2):
    from gpry_amd.nested import cholesky_ridged
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 3, len(Xs)).astype(np.int32)
    Ws = []
    for q in range(3):
        A = rng.normal(size=(d, d))
        Ws.append(cholesky_ridged((0.02 + 0.05 * q) * (A @ A.T / d + 0.1 * np.eye(d))))
    return labels, np.stack(Ws)


def test_volumes_chain_equals_the_unclustered_chain_on_its_clusters_survivors():
    from gpry_amd.nested import chain_clusters
    d, k = 5, 128
    gpr, lo, hi, Xs, ys, lstar = _generation_inputs(d, 4)
    labels, W = _three_clusters(d, Xs)
    cum_p = np.array([0.15, 0.55, 1.0])
    Xc, yc, cc, _ = gpr.device.ns_generation(lo, hi, Xs, ys, lstar, W, 21, 7, k, 10, labels=labels, cum_p=cum_p)
    q = chain_clusters(21, 7, k, cum_p)
    np.testing.assert_array_equal(q, ns_volumes.drawn_clusters(21, 7, k, cum_p))
    assert set(q.tolist()) == {0, 1, 2}
    for c in range(3):
        mem = np.flatnonzero(labels == c)
        Xq, yq, cq, _ = gpr.device.ns_generation(lo, hi, Xs[mem], ys[mem], lstar, W[c], 21, 7, k, 10)
        sel = q == c
        np.testing.assert_array_equal(Xc[sel], Xq[sel])
        np.testing.assert_array_equal(yc[sel], yq[sel])
        np.testing.assert_array_equal(cc[sel], cq[sel])
    np.testing.assert_array_equal(yc, _one_point(gpr, Xc))
    assert np.all(yc > lstar)


def test_drawn_clusters_and_starts_match_the_host_and_follow_cum_p():
    """With no steps a chain returns its start, so the device's cluster and start draws can be read off directly."""
    from gpry_amd.nested import chain_clusters
    d, k = 3, 20000
    gpr, lo, hi, Xs, ys, lstar = _generation_inputs(d, 5)
    labels, W = _three_clusters(d, Xs, seed=3)
    cum_p = np.array([0.1, 0.1, 1.0])                  # cluster 1 has probability 0: never drawn
    X0, y0, c0, _ = gpr.device.ns_generation(lo, hi, Xs, ys, lstar, W, 33, 2, k, 0, labels=labels, cum_p=cum_p)
    assert not c0.any()
    index = {tuple(x): i for i, x in enumerate(Xs)}
    start = np.array([index[tuple(x)] for x in X0])
    q = chain_clusters(33, 2, k, cum_p)
    np.testing.assert_array_equal(labels[start], q)
    # the start among q's survivors in their order: min(floor(u0 n_q), n_q - 1) with the unclustered u0
    u0, _ = ns_volumes.philox(33, ns_volumes.PHASE_START, 0, 2, np.arange(k), 0)
    for c in (0, 2):
        mem = np.flatnonzero(labels == c)
        sel = q == c
        np.testing.assert_array_equal(start[sel], mem[np.minimum((u0[sel] * len(mem)).astype(np.int64), len(mem) - 1)])
    np.testing.assert_array_equal(y0, ys[start])
    freq = np.bincount(q, minlength=3) / k
    p = np.diff(np.concatenate([[0.0], cum_p]))
    assert freq[1] == 0.0 and np.all(np.abs(freq - p) < 4 * np.sqrt(p * (1 - p) / k) + 1e-12), freq


def test_invalid_inputs_are_refused_and_the_context_stays_usable():
    from gpry_amd._lib import GpryHipError
    d = 3
    gpr, lo, hi, Xs, ys, lstar = _generation_inputs(d, 6)
    labels = (np.arange(len(Xs)) % 3).astype(np.int32)
    W = np.stack([0.1 * np.eye(d)] * 3)
    good = np.array([0.2, 0.6, 1.0])

    def call(lab, cp):
        return gpr.device.ns_generation(lo, hi, Xs, ys, lstar, W, 1, 0, 8, 2, labels=lab, cum_p=cp)

    want = call(labels, good)
    for v in (3, -1):
        bad = labels.copy()
        bad[4] = v
        with pytest.raises(GpryHipError, match="gpry_ns_generation_volumes.*labels"):
            call(bad, good)
    for cp, msg in (([0.6, 0.2, 1.0], "non-decreasing"), ([0.2, np.nan, 1.0], "non-decreasing"),
                    ([-0.1, 0.6, 1.0], "non-decreasing"), ([0.2, 0.6, 0.999], "not 1.0")):
        with pytest.raises(GpryHipError, match=f"gpry_ns_generation_volumes.*{msg}"):
            call(labels, np.array(cp))
    empty = labels.copy()
    empty[empty == 1] = 0
    with pytest.raises(GpryHipError, match="gpry_ns_generation_volumes.*no survivor"):
        call(empty, good)
    call(empty, np.array([0.2, 0.2, 1.0]))            # an empty cluster of probability 0 is fine
    got = call(labels, good)
    for u, v in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(u, v)


def test_same_seed_same_bits_on_two_contexts_with_volumes():
    d = 2
    gpr, bounds = _fitted_bimodal(d, 200)
    kw = dict(nlive=100, num_repeats=5 * d, nprior=1000, clustering=True, cluster_volumes=True)
    a = _run(gpr, bounds, 5, **kw)
    b = _run(gpr, bounds, 5, **kw)
    gpr2, _ = _fitted_bimodal(d, 200)
    assert gpr2.device is not gpr.device
    c = _run(gpr2, bounds, 5, **kw)
    assert a.n_clusters.max() >= 2 and len(a.cluster_parent) >= 3
    for o in (b, c):
        for f in ("X", "y", "w", "n_clusters", "cluster", "cluster_logZ", "cluster_parent"):
            np.testing.assert_array_equal(getattr(o, f), getattr(a, f), err_msg=f)
        assert o.logZ == a.logZ and o.ncalls == a.ncalls


@pytest.mark.timeout(900)
def test_bimodal_surrogate_mode_evidences_against_quadrature():
    """nlive = 50 d (the clustered test without volumes needs 1000 d for its mass bound): profiles/nested_volumes.md."""
    d = 4
    gpr, bounds = _fitted_bimodal(d, 500)
    n = 40
    logZq, _, _ = _quadrature(gpr, bounds, n)
    axes = [bounds[k, 0] + (np.arange(n) + 0.5) * (bounds[k, 1] - bounds[k, 0]) / n for k in range(d)]
    G = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    yg = gpr.predict(G)
    pg = np.exp(yg - yg.max())
    frac_q = np.sum(pg[G[:, 0] < 0]) / np.sum(pg)
    for seed in (1, 2, 3):
        nlive = 50 * d
        r = _run(gpr, bounds, seed, nlive=nlive, num_repeats=5 * d, nprior=10 * nlive, clustering=True,
                 cluster_volumes=True)
        _check_bookkeeping(r, nlive)
        assert r.n_clusters.max() >= 2
        assert abs(r.logZ - logZq) < 4 * r.logZ_err, (seed, r.logZ, logZq, r.logZ_err)
        left, right = _mode_logZ(r)
        assert abs(left - (logZq + np.log(frac_q))) < 5 * r.logZ_err, (seed, left, frac_q)
        assert abs(right - (logZq + np.log(1 - frac_q))) < 5 * r.logZ_err, (seed, right, frac_q)
        # the mass of a mode at this nlive: 0.22 .. 0.55 against 0.40 over 16 seeds (profiles/nested_volumes.md)
        assert abs(np.exp(left - r.logZ) - frac_q) < 0.2, (seed, np.exp(left - r.logZ), frac_q)


@pytest.mark.timeout(900)
def test_multi_add_with_volumes_matches_the_oracle():
    from gpry_amd.gp_acquisition import NORA
    d, N, npts = 4, 512, 4
    ll = _bimodal_ll(d)
    rng = np.random.default_rng(3)
    m = np.zeros(d)
    m[0] = 2.0
    X = np.clip(np.concatenate([rng.uniform(-4, 4, (N // 2, d)), rng.normal(-m, 0.6, (N // 4, d)),
                                rng.normal(m, 0.5, (N // 4, d))]), -4, 4)
    y = ll(X)
    bounds = np.array([[-4.0, 4.0]] * d)
    theta = np.log([4.0] + [0.6] * d)
    gpr = make_gpr(bounds, orc.MATERN52, theta=theta)
    gpr.append_to_data(X, y, fit_gpr=False)
    ref = orc.OracleGPR(bounds, kernel_id=orc.MATERN52)
    ref.theta = theta.copy()
    ref.fitted = True
    ref.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    acq = NORA(bounds, sampler="nested", verbose=0, devices=[0], nlive_max=200, shortlist_size=32,
               nested_clustering=True, nested_cluster_volumes=True)
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(4))
    info = acq.stats["sampler_info"]
    assert info["ncalls"] > 0 and info["clusters"] >= 2 and len(info["cluster_logZ"]) >= 3
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert len(Xs) == info["rows"] and abs(np.sum(ws) - 1.0) < 1e-12
    np.testing.assert_array_equal(ys[:300], _one_point(gpr, Xs[:300]))
    Xo, yo, ao, so, _ = oracle_given(ref, Xs, ys, None, npts, zeta=acq.acq_func.zeta)
    np.testing.assert_array_equal(Xp, Xo)
    np.testing.assert_allclose(yp, yo, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(ap, ao, rtol=1e-7, atol=1e-7)
