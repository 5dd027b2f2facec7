"""NORA with a sampler that returns its own y, or y and sigma_y (the three cases of the reference's
mpi.compute_y_parallel, gpry/mpi.py:182-218): dispatch, n_eval accounting, the lazy sigma-only fetch,
re-weighting against the caller's y and a two-rank sharded run -- the oracle stands in for the device."""
import os
import socket
import sys

import numpy as np
import pytest

from oracle import gpry_oracle as orc
from test_host_logic_cpu import FakeDevice, FakeGPR, _golden_model


class GivenFakeDevice(FakeDevice):
    """FakeDevice that also takes the sampler's arrays (Device.sweep_logexp(y_given=, sigma_given=))."""

    def __init__(self, model, lazy=False):
        super().__init__(model)
        self.sweep_epoch = 0
        self.calls, self.fetched = [], []
        if lazy:
            self.sweep_fetch = self._fetch

    def sweep_logexp(self, X, zeta, baseline, sigma_n, mask=None, M=None, want=(), y_given=None, sigma_given=None):
        self.sweep_epoch += 1
        self.calls.append(dict(given=y_given is not None, both=sigma_given is not None, want=tuple(want),
                               resident=X is None))
        if y_given is None:
            assert sigma_given is None
            return super().sweep_logexp(X, zeta, baseline, sigma_n, mask=mask, M=M, want=want)
        X = self._lastX if X is None else X
        self._lastX = X
        y = np.asarray(y_given, dtype=float)
        s = self.m.predict_std(X) if sigma_given is None else np.asarray(sigma_given, dtype=float)
        self.acq = orc.logexp_f(y, s, baseline, sigma_n, zeta)
        self.y, self.s = y, s
        return {"y": y, "sigma": s, "acq": self.acq, "n_nan": int(np.isnan(self.acq).sum())}

    def _fetch(self, want=("y", "sigma")):
        self.fetched.append(tuple(want))
        return {k: (getattr(self, {"y": "y", "sigma": "s", "acq": "acq"}[k]) if k in want else None)
                for k in ("y", "sigma", "acq")}


class GivenFakeGPR(FakeGPR):
    def __init__(self, model, lazy=False):
        super().__init__(model)
        self.device = GivenFakeDevice(model, lazy=lazy)
        self.mask_calls = []

    def _masks(self, X, validate, ignore):
        self.mask_calls.append(ignore)
        return None


def oracle_given(m, Xc, y, sigma, npts, zeta=None):
    """The reference's flow with the sampler's arrays: compute_y_parallel (sigma from predict_std when not given),
    LogExp.f on (y, sigma), the ranked pool (gp_acquisition.py:1049-1108)."""
    zeta = orc.auto_zeta(m.d) if zeta is None else zeta
    s = m.predict_std(Xc) if sigma is None else sigma

    def f(mu, std):
        return orc.logexp_f(mu, std, m.y_max, m.noise_level, zeta)

    acq = f(y, s)
    pool = orc.OracleRankedPool(npts, m, f)
    pool.add(Xc, y, s, acq)
    k = min(pool.filled(), npts)
    return pool.X[:k].copy(), pool.y[:k].copy(), f(pool.y[:k], pool.sigma[:k]), s, acq


def _given_y(m, Xc, seed=3):
    """A sampler's own log-posterior: the model's mean, perturbed (so that it is not what the sweep would compute)."""
    return m.predict(Xc) + 0.5 * np.random.default_rng(seed).standard_normal(len(Xc))


def _nora(bounds, sample, **kw):
    from gpry_amd.gp_acquisition import NORA
    acq = NORA(bounds, sampler="uniform", verbose=0, **kw)
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: sample
    return acq


def test_dispatch_of_the_three_cases_and_n_eval():
    g, p, bounds, Xc, m = _golden_model("a")
    M = len(Xc)
    y = _given_y(m, Xc)
    s = m.predict_std(Xc) * 1.5
    gpr = GivenFakeGPR(m)
    acq = _nora(bounds, None)
    # y is None: mean and sigma computed, counted as one predict of M points
    acq._set_MC_sample(Xc, None, None, None, ensure_y_sigma_y=True, gpr=gpr)
    assert gpr.n_eval == M and gpr.device.calls[-1]["given"] is False
    np.testing.assert_allclose(acq._y_mc, m.predict(Xc), rtol=1e-12)
    # y given: kept as the caller's object, sigma from predict_std (counted), classifier-only host mask
    acq._set_MC_sample(Xc, y, None, None, ensure_y_sigma_y=True, gpr=gpr)
    assert gpr.n_eval == 2 * M
    c = gpr.device.calls[-1]
    assert c["given"] and not c["both"] and "y" not in c["want"]
    assert gpr.mask_calls[-1] is True and gpr.mask_calls[0] is False
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert ys is y and Xs is Xc
    np.testing.assert_allclose(ss, m.predict_std(Xc), rtol=1e-12)
    # both given: nothing predicted, nothing counted, no gates
    n_masks = len(gpr.mask_calls)
    acq._set_MC_sample(Xc, y, s, None, ensure_y_sigma_y=True, gpr=gpr)
    assert gpr.n_eval == 2 * M and len(gpr.mask_calls) == n_masks
    c = gpr.device.calls[-1]
    assert c["given"] and c["both"] and c["want"] == ()
    Xs, ys, ss, ws = acq.last_MC_sample()
    assert ys is y and ss is s
    np.testing.assert_array_equal(gpr.device.acq, orc.logexp_f(y, s, m.y_max, m.noise_level, acq.acq_func.zeta))


def test_sigma_without_y_is_recomputed():
    """compute_y_parallel assumes sigma_y is None when y is: a sigma_y alone is dropped and both are computed."""
    g, p, bounds, Xc, m = _golden_model("b")
    gpr = GivenFakeGPR(m)
    junk = np.full(len(Xc), 7.0)
    acq = _nora(bounds, (Xc, None, junk, None))
    acq.multi_add(gpr, n_points=2, rng=np.random.default_rng(0))
    assert gpr.device.calls[0]["given"] is False
    _, ys, ss, _ = acq.last_MC_sample()
    np.testing.assert_allclose(ys, m.predict(Xc), rtol=1e-12)
    np.testing.assert_allclose(ss, m.predict_std(Xc), rtol=1e-12)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("with_sigma", [False, True])
def test_multi_add_with_given_arrays_equals_the_reference_flow(tag, with_sigma):
    g, p, bounds, Xc, m = _golden_model(tag)
    npts = len(g[p + "acq_cond"]) - 1
    y = _given_y(m, Xc)
    s = m.predict_std(Xc) * 0.8 if with_sigma else None
    gpr = GivenFakeGPR(m)
    acq = _nora(bounds, (Xc, y, s, None), shortlist_size=8)
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    Xo, yo, ao, so, _ = oracle_given(m, Xc, y, s, npts)
    np.testing.assert_array_equal(Xp, Xo)
    np.testing.assert_allclose(yp, yo, rtol=1e-12)
    np.testing.assert_allclose(ap, ao, rtol=1e-9)
    assert acq.last_MC_sample()[1] is y


def test_lazy_sigma_only_fetch_keeps_the_callers_y():
    g, p, bounds, Xc, m = _golden_model("a")
    y = _given_y(m, Xc)
    gpr = GivenFakeGPR(m, lazy=True)
    acq = _nora(bounds, (Xc, y, None, None))
    acq.multi_add(gpr, n_points=2, rng=np.random.default_rng(0))
    assert gpr.device.calls[0]["want"] == () and acq._sigma_y_mc is None and acq._y_mc is y
    Xs, ys, ss, _ = acq.last_MC_sample()
    assert gpr.device.fetched == [("sigma",)]
    assert ys is y
    np.testing.assert_allclose(ss, m.predict_std(Xc), rtol=1e-12)
    acq.last_MC_sample()
    assert gpr.device.fetched == [("sigma",)]          # fetched once


def test_nan_in_the_callers_y_raises():
    g, p, bounds, Xc, m = _golden_model("a")
    y = _given_y(m, Xc)
    y[5] = np.nan
    acq = _nora(bounds, (Xc, y, None, None))
    with pytest.raises(ValueError, match="not a number"):
        acq.multi_add(GivenFakeGPR(m), n_points=2, rng=np.random.default_rng(0))


def test_reweighting_uses_the_callers_y():
    """mc_every = 2: the second call re-weights the sample against the caller's y (gp_acquisition.py:875-919)."""
    g, p, bounds, Xc, m = _golden_model("b")
    npts = len(g[p + "acq_cond"]) - 1
    y = _given_y(m, Xc)
    gpr = GivenFakeGPR(m)
    acq = _nora(bounds, (Xc, y, None, None), mc_every=2)
    Xp, _, _ = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    gpr.append_to_data(Xp, g[p + "y_new"])
    acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
    assert acq.is_last_MC_reweighted
    with np.errstate(all="ignore"):
        w = np.exp(m.predict(Xc) - y)
    w /= w.max()
    keep = w != 0
    Xr, yr, sr, wr = acq.last_MC_sample(warn_reweight=False)
    np.testing.assert_array_equal(Xr, Xc[keep])
    np.testing.assert_allclose(wr, w[keep], rtol=1e-9)
    np.testing.assert_allclose(yr, m.predict(Xc)[keep], rtol=1e-12)


def _worker(rank, world, port, tag, q):
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_multirank_cpu import GlooComm
        g, p, bounds, Xc, m = _golden_model(tag)
        npts = len(g[p + "acq_cond"]) - 1
        y = _given_y(m, Xc)
        gpr = GivenFakeGPR(m)
        comm = GlooComm()
        acq = _nora(bounds, (Xc, y, None, None), mc_every=2, comm=comm, shortlist_size=8)
        Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(2))
        lo, hi = acq._sweep_lo, acq._sweep_hi
        _, ys, ss, _ = acq.last_MC_sample()
        q.put((rank, Xp, yp, ap, ys is y, ss, len(gpr.device.acq), (lo, hi)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_two_rank_sweep_of_the_callers_y_equals_one_rank(tag):
    mp = pytest.importorskip("torch.multiprocessing")
    g, p, bounds, Xc, m = _golden_model(tag)
    npts = len(g[p + "acq_cond"]) - 1
    y = _given_y(m, Xc)
    one = _nora(bounds, (Xc, y, None, None), mc_every=2, shortlist_size=8)
    X1, y1, a1 = one.multi_add(GivenFakeGPR(m), n_points=npts, rng=np.random.default_rng(2))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    procs = [ctx.Process(target=_worker, args=(r, world, port, tag, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    shards = []
    for rank, Xp, yp, ap, same_y, ss, n_swept, (lo, hi) in res:
        np.testing.assert_array_equal(Xp, X1)
        np.testing.assert_array_equal(yp, y1)
        np.testing.assert_allclose(ap, a1, rtol=1e-12)
        assert same_y
        assert n_swept == hi - lo < len(Xc)            # each rank swept its slice of the caller's y
        np.testing.assert_allclose(ss, m.predict_std(Xc), rtol=1e-12)     # sigma all-gathered
        shards.append((lo, hi))
    assert shards[0][0] == 0 and shards[0][1] == shards[1][0] and shards[1][1] == len(Xc)
