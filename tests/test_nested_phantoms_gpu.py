"""Phantom points of the nested sampler on the device (gpry_ns_generation_phantoms, ns_chain_kernel's recording): slot i of
a chain equals, bit for bit, the last point of the same chain walked for (i + 1) thin steps by the existing entry points,
in the unclustered, clustered and volume-drawn modes and in all four dimension buckets; its own last points are those of
the existing entry points; every recorded y is gpr.predict of its row alone with the gates on; run_nested with phantoms
is the run without plus rows; NORA ranks the grown pool; the entry point's refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_nested_cluster_gpu import _generation_inputs
from test_nested_gpu import _fitted, _fixed, _gauss_ll, _one_point, _run, _svm_model
from test_nested_volumes_gpu import _three_clusters

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

pytestmark = pytest.mark.gpu

R, K = 7, 48


@functools.lru_cache(maxsize=None)
def _inputs(d):
    return _generation_inputs(d, 3 + d)


def _mode_kw(mode, d, Xs, lo, hi):
    from gpry_amd.nested import whitening
    if mode == "plain":
        return whitening((Xs - lo) / (hi - lo)), {}
    labels, W = _three_clusters(d, Xs)
    if mode == "labels":
        return W, {"labels": labels}
    return W, {"labels": labels, "cum_p": np.array([0.15, 0.55, 1.0])}


@pytest.mark.parametrize("mode", ["plain", "labels", "labels + cum_p"])
@pytest.mark.parametrize("thin", [1, 3])
@pytest.mark.parametrize("d", [3, 8, 13, 20])
def test_every_slot_is_the_shorter_chains_last_point(d, thin, mode):
    gpr, lo, hi, Xs, ys, lstar = _inputs(d)
    dev = gpr.device
    W, kw = _mode_kw(mode, d, Xs, lo, hi)
    seed, gen = 21 + d, 7
    Xn, yn, cn, Xp, yp, ms = dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, seed, gen, K, R, thin, **kw)
    n_ph = (R - 1) // thin
    assert Xp.shape == (K, n_ph, d) and yp.shape == (K, n_ph) and ms > 0
    full = dev.ns_generation(lo, hi, Xs, ys, lstar, W, seed, gen, K, R, **kw)
    np.testing.assert_array_equal(Xn, full[0])
    np.testing.assert_array_equal(yn, full[1])
    np.testing.assert_array_equal(cn, full[2])
    moved = False
    for i in range(n_ph):
        Xi, yi, _, _ = dev.ns_generation(lo, hi, Xs, ys, lstar, W, seed, gen, K, (i + 1) * thin, **kw)
        np.testing.assert_array_equal(Xp[:, i], Xi, err_msg=f"slot {i}")
        np.testing.assert_array_equal(yp[:, i], yi, err_msg=f"slot {i}")
        moved = moved or (i > 0 and not np.array_equal(Xp[:, i], Xp[:, i - 1]))
    assert moved and np.all(yp > lstar)
    assert np.all((Xp >= lo) & (Xp <= hi))


def test_no_slot_and_no_buffers():
    """thin >= num_repeats leaves nothing to record; num_repeats 0 and 1 likewise; the call is then the plain one."""
    gpr, lo, hi, Xs, ys, lstar = _inputs(3)
    dev = gpr.device
    W, _ = _mode_kw("plain", 3, Xs, lo, hi)
    for reps, thin in ((R, R), (R, 50), (1, 1), (0, 1)):
        out = dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 5, 2, K, reps, thin)
        assert out[3].shape == (K, 0, 3) and out[4].shape == (K, 0)
        for u, v in zip(out[:3], dev.ns_generation(lo, hi, Xs, ys, lstar, W, 5, 2, K, reps)[:3]):
            np.testing.assert_array_equal(u, v)


def test_recorded_y_is_one_point_predict_with_the_gates_on():
    gpr, bounds = _svm_model()
    gpr._ensure_factor()
    gpr._push_affine()
    assert gpr._push_gates()
    from gpry_amd.nested import whitening
    lo, hi = bounds[:, 0].copy(), bounds[:, 1].copy()
    X, y, _ = gpr.device.ns_prior(lo, hi, 4, 400)
    assert np.any(np.isinf(y))                       # some of the prior is on rejected ground
    order = np.argsort(y)
    Xs, ys, lstar = X[order[250:]], y[order[250:]], float(y[order[249]])
    assert np.isfinite(lstar)
    W = whitening((Xs - lo) / (hi - lo))
    Xn, yn, cn, Xp, yp, _ = gpr.device.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 8, 1, 64, 9, 2)
    rows = np.random.default_rng(0).choice(64 * 4, 120, replace=False)
    np.testing.assert_array_equal(yp.reshape(-1)[rows], _one_point(gpr, Xp.reshape(-1, 3)[rows]))
    np.testing.assert_array_equal(yn, _one_point(gpr, Xn))
    assert np.all(yp > lstar)


@pytest.mark.parametrize("clustering", [False, True])
def test_run_with_phantoms_is_the_run_without_plus_rows(clustering):
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, np.log([4.0, 0.3, 0.3, 0.3, 0.3]))
    kw = dict(nlive=80, num_repeats=8, nprior=400, clustering=clustering)
    a = _run(gpr, bounds, 5, **kw)
    b = _run(gpr, bounds, 5, phantom_thin=2, **kw)
    n = len(a.y)
    assert b.n_phantom == b.ngen * 40 * 3 > 0 and len(b.y) == n + b.n_phantom
    np.testing.assert_array_equal(b.X[:n], a.X)
    np.testing.assert_array_equal(b.y[:n], a.y)
    assert b.logZ == a.logZ and b.logZ_err == a.logZ_err and b.ncalls == a.ncalls and b.ngen == a.ngen
    np.testing.assert_array_equal(b.dead_L, a.dead_L)
    np.testing.assert_array_equal(b.dead_logX, a.dead_logX)
    assert np.all(b.w >= 0) and abs(np.sum(b.w) - 1.0) < 1e-12 and len(b.w) == len(b.y)
    rows = n + np.random.default_rng(1).choice(b.n_phantom, 150, replace=False)
    np.testing.assert_array_equal(b.y[rows], _one_point(gpr, b.X[rows]))
    assert np.all((b.X >= bounds[:, 0]) & (b.X <= bounds[:, 1]))
    assert np.isfinite(b.logZ_merged)
    assert 1.0 / np.sum(b.w ** 2) > 1.0 / np.sum(a.w ** 2)


@pytest.mark.timeout(900)
def test_multi_add_ranks_the_pool_with_its_phantoms():
    from gpry_amd.gp_acquisition import NORA
    gpr, bounds = _fitted(_gauss_ll(3), 3, 200)
    kw = dict(sampler="nested", verbose=0, devices=[0], nlive_max=150, shortlist_size=32)
    off = NORA(bounds, **kw)
    off.multi_add(gpr, n_points=3, rng=np.random.default_rng(4))
    acq = NORA(bounds, nested_phantoms=2, **kw)
    Xp, yp, ap = acq.multi_add(gpr, n_points=3, rng=np.random.default_rng(4))
    info, info0 = acq.stats["sampler_info"], off.stats["sampler_info"]
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert info["phantom_thin"] == 2 and info["phantom_rows"] > 0 and np.isfinite(info["logZ_merged"])
    assert info["rows"] == len(Xs) == info0["rows"] + info["phantom_rows"]
    assert info["logZ"] == info0["logZ"] and info["ncalls"] == info0["ncalls"]
    assert len(ws) == len(Xs) and abs(np.sum(ws) - 1.0) < 1e-12 and np.all(ws >= 0)
    assert len(Xp) == 3
    pool = {tuple(x) for x in Xs}
    assert all(tuple(x) in pool for x in Xp)
    rows = np.random.default_rng(2).choice(len(Xs), 200, replace=False)
    np.testing.assert_array_equal(ys[rows], _one_point(gpr, Xs[rows]))


def test_refusals_of_the_entry_point_leave_the_context_usable():
    from gpry_amd._lib import GpryHipError, _ptr
    gpr, lo, hi, Xs, ys, lstar = _inputs(3)
    dev = gpr.device
    W, _ = _mode_kw("plain", 3, Xs, lo, hi)
    want = dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 1, 0, 8, 4, 1)
    for thin in (0, -3):
        with pytest.raises(GpryHipError, match="gpry_ns_generation_phantoms.*thin"):
            dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 1, 0, 8, 4, thin)
    # exactly one of X_ph / y_ph
    Xn, yn, cn = np.empty((8, 3)), np.empty(8), np.zeros(8, np.int64)
    Xph, yph, ms = np.empty((8, 3, 3)), np.empty((8, 3)), C.c_double(0.0)
    Xsc, ysc = np.ascontiguousarray(Xs), np.ascontiguousarray(ys)

    def raw(px, py, thin=1):
        return dev._lib.gpry_ns_generation_phantoms(dev._h, _ptr(lo), _ptr(hi), _ptr(Xsc), _ptr(ysc), len(Xsc),
                                                    float(lstar), _ptr(W), 1, 0, 8, 4, None, 1, None, _ptr(Xn), _ptr(yn),
                                                    _ptr(cn), thin, px, py, C.byref(ms))

    for px, py in ((_ptr(Xph), None), (None, _ptr(yph))):
        assert raw(px, py) == -1
        assert b"X_ph and y_ph" in dev._lib.gpry_last_error(dev._h)
    assert raw(None, None, thin=0) == -1                               # thin is checked without buffers too
    assert raw(None, None) == 0                                        # both NULL: the plain generation
    np.testing.assert_array_equal(Xn, want[0])
    assert raw(_ptr(Xph), _ptr(yph)) == 0
    np.testing.assert_array_equal(Xph, want[3])
    np.testing.assert_array_equal(yph, want[4])
    # more than 2^30 bytes of phantoms: 70000 chains x 500 states x (3 + 1) doubles
    with pytest.raises(GpryHipError, match="gpry_ns_generation_phantoms.*limit"):
        dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 1, 0, 70000, 501, 1)
    # cum_p without labels, as the other entry points refuse it
    assert dev._lib.gpry_ns_generation_phantoms(dev._h, _ptr(lo), _ptr(hi), _ptr(Xsc), _ptr(ysc), len(Xsc), float(lstar),
                                                _ptr(W), 1, 0, 8, 4, None, 1, _ptr(np.array([1.0])), _ptr(Xn), _ptr(yn),
                                                _ptr(cn), 1, _ptr(Xph), _ptr(yph), C.byref(ms)) == -1
    got = dev.ns_generation_phantoms(lo, hi, Xs, ys, lstar, W, 1, 0, 8, 4, 1)
    for u, v in zip(got[:5], want[:5]):
        np.testing.assert_array_equal(u, v)
