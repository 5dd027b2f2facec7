"""The nested sampler's host loop (gpry_amd/nested.py) driven by the numpy stand-in of its two device calls
(tests/tools/ns_philox.py), and NORA's sampler="nested" path with the oracle standing in for the device: evidence of an
analytic Gaussian, the invariants of the dead sequence and the volumes, the settings of update_NS_precision, the seed,
max_ncalls, the hand-over of y to the given-y sweep and the refusal of a classifier without a device form."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_given_y_cpu import GivenFakeDevice, GivenFakeGPR, oracle_given
from test_host_logic_cpu import _golden_model

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_philox  # noqa: E402


def _gauss(d, mu=0.3, s=0.5):
    """Normalised Gaussian log-density; with the box [-4, 4]^d its evidence against the uniform prior is -d log 8."""
    def loglike(X):
        X = np.atleast_2d(X)
        return -0.5 * np.sum((X - mu) ** 2, axis=1) / s ** 2 - 0.5 * d * np.log(2 * np.pi * s ** 2)
    return loglike, np.array([[-4.0, 4.0]] * d), -d * np.log(8.0)


@pytest.mark.parametrize("d", [2, 5])
def test_evidence_of_an_analytic_gaussian(d):
    from gpry_amd.nested import run_nested
    loglike, bounds, logZ = _gauss(d)
    for seed in (1, 2):
        r = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, seed, nlive=25 * d, num_repeats=5 * d,
                       precision_criterion=0.01, nprior=250 * d)
        assert abs(r.logZ - logZ) < 4 * r.logZ_err, (r.logZ, logZ, r.logZ_err)
        # the weighted mean of the posterior
        m = np.average(r.X, weights=r.w, axis=0)
        assert np.all(np.abs(m - 0.3) < 0.15), m


def test_dead_sequence_weights_and_volumes():
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(3)
    # a third of the box is "outside" (y = -inf): those points must die first and carry no weight
    def ll(X):
        y = loglike(X)
        y[X[:, 0] > 2.0] = -np.inf
        return y
    nlive, nprior, k = 40, 200, 10
    dev = ns_philox.NumpyNestedDevice(ll)
    r = run_nested(dev, bounds, 7, nlive=nlive, num_repeats=6, nprior=nprior, batch=k)
    assert np.all(r.dead_L[1:] >= r.dead_L[:-1])
    assert np.all(r.w >= 0) and abs(np.sum(r.w) - 1.0) < 1e-12
    assert np.all(np.isfinite(r.y)) and len(r.y) == len(r.X) == len(r.w)
    assert np.all((r.X >= bounds[:, 0]) & (r.X <= bounds[:, 1]))
    # volumes: one factor n / (n + 1) per removal, n = the live count before it
    n_before = list(range(nprior, nlive, -1)) + [nlive - j for _ in range(r.ngen) for j in range(k)]
    assert r.n_dead == len(n_before)
    np.testing.assert_allclose(r.dead_logX, np.cumsum(np.log(np.array(n_before) / (np.array(n_before) + 1.0))),
                               rtol=1e-13)
    # every generation's L* is its largest removed value; the chains' new points lie above it
    assert [c["k"] for c in dev.calls] == [k] * r.ngen
    for g, c in enumerate(dev.calls):
        assert c["lstar"] == r.dead_L[nprior - nlive + (g + 1) * k - 1]
    # rows: the finite dead points in order of death, then the final live points
    fin = np.isfinite(r.dead_L)
    assert len(r.y) == int(fin.sum()) + nlive


def test_max_ncalls_stops_the_run():
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(2)
    dev = ns_philox.NumpyNestedDevice(loglike)
    full = run_nested(dev, bounds, 3, nlive=50, num_repeats=10, nprior=200)
    cap = 200 + 3000
    r = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, 3, nlive=50, num_repeats=10, nprior=200, max_ncalls=cap)
    assert r.ngen < full.ngen
    assert r.ncalls >= cap
    # a generation of 25 chains makes at most 10 steps x (2 x 32 + 64) evaluations each
    assert r.ncalls < cap + 25 * 10 * 128
    assert r.ngen >= 1


def test_same_seed_same_run_other_seed_other_run():
    from gpry_amd.nested import run_nested
    loglike, bounds, _ = _gauss(2)
    a = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, 11, nlive=30, num_repeats=6, nprior=90)
    b = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, 11, nlive=30, num_repeats=6, nprior=90)
    c = run_nested(ns_philox.NumpyNestedDevice(loglike), bounds, 12, nlive=30, num_repeats=6, nprior=90)
    assert np.array_equal(a.X, b.X) and np.array_equal(a.w, b.w) and a.logZ == b.logZ
    assert not np.array_equal(a.X[:10], c.X[:10])


def test_philox_restatement_matches_the_known_answers():
    """Philox4x32-10 known-answer vectors (Salmon et al. 2011): the words behind the first uniform."""
    u, _ = ns_philox.philox(0, 0, 0, 0, 0, 0)
    assert int(u * 2.0 ** 53) == ((0x6627e8d5 << 32) | 0xe169c58d) >> 11
    u, v = ns_philox.philox(0xFFFFFFFFFFFFFFFF, 0xFF, 0xFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert int(u * 2.0 ** 53) == ((0x408f276d << 32) | 0x41c83b0e) >> 11
    assert int(v * 2.0 ** 53) == ((0xa20bc7c6 << 32) | 0x6d5451fd) >> 11


# ---- NORA ---------------------------------------------------------------------------------------------------------
class NestedFakeDevice(GivenFakeDevice):
    """The given-y sweep of the oracle plus the two sampler calls on the model's mean."""

    def __init__(self, model):
        super().__init__(model)
        self.ns = ns_philox.NumpyNestedDevice(lambda X: model.predict(X))
        self.ns_prior, self.ns_generation = self.ns.ns_prior, self.ns.ns_generation


class NestedFakeGPR(GivenFakeGPR):
    minus_inf_value = -np.inf

    def __init__(self, model, device_gates=True):
        super().__init__(model)
        self.device = NestedFakeDevice(model)
        self.device_gates = device_gates
        self.gate_pushes = 0

    def _push_gates(self, ignore_trust_region=False, sinks=None):
        self.gate_pushes += 1
        return self.device_gates


def test_update_NS_precision_settings_and_seed_reach_the_sampler(monkeypatch):
    from gpry_amd import nested
    from gpry_amd.gp_acquisition import NORA
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = NestedFakeGPR(m)
    acq = NORA(bounds, sampler="nested", verbose=0, nlive_per_training=2, nlive_max=40, num_repeats=7,
               precision_criterion_target=0.05, nprior_per_nlive=3, max_ncalls=5000, nested_batch=6)
    seen = {}
    real = nested.run_nested

    def spy(dev, b, seed, nlive, num_repeats, **kw):
        seen.update(dev=dev, bounds=b, seed=seed, nlive=nlive, num_repeats=num_repeats, **kw)
        return real(dev, b, seed, nlive, num_repeats, **kw)

    monkeypatch.setattr(nested, "run_nested", spy)
    X, y, s, w = acq.do_MC_sample(gpr, None, rng=np.random.default_rng(5))
    prec = acq.update_NS_precision(gpr)
    assert prec["nlive"] == min(2 * m.n, 40)
    assert seen["nlive"] == prec["nlive"] and seen["num_repeats"] == 7
    assert seen["precision_criterion"] == 0.05 and seen["nprior"] == 3 * prec["nlive"]
    assert seen["max_ncalls"] == 5000 and seen["batch"] == 6
    assert seen["seed"] == np.random.default_rng(5).integers(2**31 - 1)
    assert seen["dev"] is gpr.device and np.array_equal(seen["bounds"], np.asarray(bounds, dtype=float))
    assert s is None and len(X) == len(y) == len(w)
    np.testing.assert_allclose(y, m.predict(X), rtol=1e-12)   # (the oracle's batched mean: bits depend on the batch)
    info = acq.stats["sampler_info"]
    assert info["ncalls"] >= 3 * prec["nlive"] and info["seed"] == seen["seed"] and info["generations"] >= 0
    assert gpr.gate_pushes == 1


def test_nora_nested_hands_y_to_the_given_y_sweep():
    from gpry_amd.gp_acquisition import NORA
    g, p, bounds, Xc, m = _golden_model("b")
    npts = 3
    gpr = NestedFakeGPR(m)
    acq = NORA(bounds, sampler="nested", verbose=0, nlive_max=30, num_repeats=4, nprior_per_nlive=3)
    n0 = gpr.n_eval
    Xp, yp, ap = acq.multi_add(gpr, n_points=npts, rng=np.random.default_rng(9))
    c = gpr.device.calls[-1]
    assert c["given"] and not c["both"]
    X, y, s, w = acq.last_MC_sample()
    np.testing.assert_allclose(y, m.predict(X), rtol=1e-12)   # (the oracle's batched mean: bits depend on the batch)
    assert w is not None and abs(np.sum(w) - 1) < 1e-12
    info = acq.stats["sampler_info"]
    assert gpr.n_eval - n0 >= info["ncalls"]
    Xr, yr, ar, _, _ = oracle_given(m, X, y, None, npts)
    np.testing.assert_array_equal(Xp, Xr)
    np.testing.assert_allclose(ap, ar, rtol=1e-9)


def test_classifier_without_device_form_is_refused():
    from gpry_amd.gp_acquisition import NORA
    g, p, bounds, Xc, m = _golden_model("a")
    gpr = NestedFakeGPR(m, device_gates=False)
    acq = NORA(bounds, sampler="nested", verbose=0)
    with pytest.raises(ValueError, match="uniform") as e:
        acq.multi_add(gpr, n_points=1, rng=np.random.default_rng(1))
    assert "do_MC_sample" in str(e.value)


def test_sampler_names():
    from gpry_amd.gp_acquisition import NORA, NestedSamplerNotInstalledError
    bounds = np.array([[0.0, 1.0]] * 2)
    assert NORA(bounds, verbose=0).sampler == "uniform"
    assert NORA(bounds, sampler="nested", verbose=0).sampler == "nested"
    with pytest.raises(NestedSamplerNotInstalledError):
        NORA(bounds, sampler="polychord", verbose=0)
