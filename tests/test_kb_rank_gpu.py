"""gpry_kb_rank on the GPU against the Python path on the same context (option "kb_rank" = 0): the same picks in the
same order, the same cache_counter, acq_cond to 1e-12; a batched Gram launch against gpry_kb_gram row by row; the cases
the native path leaves to Python; one context against a group of two."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import gpry_oracle as orc
from test_host_mirror_gpu import make_gpr

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kb_rank_common as kc  # noqa: E402

pytestmark = pytest.mark.gpu

M_POOL = 3000


def _model(bounds, theta, noise_level):
    return make_gpr(bounds, 3, theta=theta, noise_level=noise_level)


def _multi_add(gpr, bounds, Xc, n_points, native, devices=(0,), trust=None):
    from gpry_amd.gp_acquisition import NORA
    gpr.device.set_option("kb_rank", int(native))
    gpr._kb = None
    acq = NORA(bounds, sampler="uniform", mc_every=1, verbose=0, shortlist_size=8, devices=list(devices))
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
    out = acq.multi_add(gpr, n_points=n_points, bounds=trust, rng=np.random.default_rng(2))
    gpr.device.set_option("kb_rank", 1)
    return acq, out


CASES = [(N, d, n_points, seed) for N in (130, 300) for d in (2, 5) for n_points in (1, 3, 8) for seed in (1, 2)]


def test_native_ranking_equals_the_python_path(monkeypatch):
    import gpry_amd.gp_acquisition as gpa
    monkeypatch.setattr(gpa, "RankedPool", kc.TrackedPool)
    n_reordered = n_tied = n_extended = 0
    models = {}
    for N, d, n_points, seed in CASES:
        if (N, d) not in models:
            models[N, d] = kc.long_scale_model(_model, N, d, seed=100 + N + d)
        bounds, gpr = models[N, d]
        Xc = np.random.default_rng(seed).uniform(bounds[:, 0], bounds[:, 1], size=(M_POOL, d))
        ref_acq, ref_out = _multi_add(gpr, bounds, Xc, n_points, native=False)
        assert ref_acq.stats["rank_native"] is False
        _, y_all, s_all, _ = ref_acq.last_MC_sample(copy=True, warn_reweight=False)    # (while the sweep is resident)
        if ref_acq.pool.near_tie:
            n_tied += 1
            continue
        nat_acq, nat_out = _multi_add(gpr, bounds, Xc, n_points, native=True)
        assert nat_acq.stats["rank_native"] is True
        what = f"N={N} d={d} n_points={n_points} seed={seed}"
        kc.assert_same_ranking(nat_acq.pool, ref_acq.pool, what)
        assert nat_acq.stats["shortlist"] == ref_acq.stats["shortlist"], what
        for a, b in zip(nat_out, ref_out):
            np.testing.assert_array_equal(a, b, err_msg=what)
        n_extended += ref_acq.stats["shortlist"] > 8
        k = kc.filled(ref_acq.pool)
        with np.errstate(divide="ignore"):
            best = np.sort(ref_acq.acq_func_y_sigma(y_all, s_all))[::-1][:k]
        n_reordered += not np.array_equal(ref_acq.pool.acq[:k], best)
    print(f"{len(CASES)} cases, {n_reordered} reordered, {n_tied} with a near-tie, {n_extended} extended the shortlist")
    assert n_extended >= 1
    assert n_tied <= 0.05 * len(CASES)
    assert n_reordered >= 0.5 * len(CASES)


def test_a_batched_gram_launch_equals_kb_gram_row_by_row():
    for N, d in ((130, 2), (300, 5)):
        bounds, gpr = kc.long_scale_model(_model, N, d, seed=7)
        Xc = np.random.default_rng(3).uniform(bounds[:, 0], bounds[:, 1], size=(301, d))
        sess = gpr.kb_session()
        sess.register(Xc)
        dev, n = gpr.device, sess.n
        rows = np.array([0, 300, 17, 17, 64, 65, 128, 255, 256, 299] + list(range(100, 170)))    # > 64 rows: two launches
        G, kv = dev.kb_gram_rows(rows, n)
        for j, p in enumerate(rows):
            g1, k1 = dev.kb_gram(int(p), n)
            assert np.array_equal(G[j], g1) and np.array_equal(kv[j], k1), (N, d, p)
        with pytest.raises(Exception):
            dev.kb_gram_rows(np.array([n]), n)


def test_a_model_with_a_classifier_is_ranked_by_the_python_path():
    bounds, X, y, Xc = orc.synthetic_like_goldens(150, 3, 400, seed=9)
    y = y.copy()
    y[X[:, 0] > 1.0] = -np.inf
    gpr = make_gpr(bounds, 3, theta=np.log(np.array([4.0, 0.3, 0.3, 0.3])), account_for_inf="SVM", inf_threshold="20s",
                   trust_region_factor=1.5, random_state=1)
    gpr.append_to_data(X, y, fit_gpr=False)
    res = []
    for native in (True, False):
        acq, out = _multi_add(gpr, bounds, Xc, 4, native=native, trust=gpr.trust_bounds)
        assert acq.stats["rank_native"] is False
        res.append(out + (acq.pool.acq_cond.copy(), acq.pool.cache_counter))
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_one_context_against_a_group_of_two():
    bounds, gpr = kc.long_scale_model(_model, 300, 5, seed=11)
    Xc = np.random.default_rng(5).uniform(bounds[:, 0], bounds[:, 1], size=(M_POOL, 5))
    res = []
    for devices in ((0,), (0, 0)):
        acq, out = _multi_add(gpr, bounds, Xc, 8, native=True, devices=devices)
        assert acq.stats["rank_native"] is True and acq.stats["sweep_contexts"] == len(devices)
        res.append(out + (acq.pool.acq_cond.copy(),))
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
