"""The Metropolis sampler's host loop (gpry_amd/mcmc.py) driven by the numpy stand-in of its device call
(tests/tools/mcmc_numpy.py), and the public calls on top of it (gpry_amd/mc.py, SmallChainProposer, patch_gpry_mc) with
a stand-in model: R - 1 against a direct restatement, the adaptation schedule, the three stopping rules, the burn-in and
the temperature weights, the options, the output file and the argument errors."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mcmc_numpy  # noqa: E402
import ns_philox  # noqa: E402


def _gauss(d, mu=0.3, s=0.5):
    def loglike(X):
        return -0.5 * np.sum((np.atleast_2d(X) - mu) ** 2, axis=1) / s ** 2
    return loglike, np.array([[-4.0, 4.0]] * d)


def _training(loglike, d, n=100, seed=0):
    X = np.random.default_rng(seed).uniform(-4, 4, (n, d))
    return X, loglike(X)


class Keeper(mcmc_numpy.NumpyMCMCDevice):
    """The stand-in, keeping what every call returned."""

    def __init__(self, loglike):
        super().__init__(loglike)
        self.outs = []

    def mcmc_chains(self, *a, **k):
        out = super().mcmc_chains(*a, **k)
        self.outs.append(out)
        return out


# ---- R - 1 --------------------------------------------------------------------------------------------------------
def test_rminus1_against_a_direct_restatement():
    from gpry_amd.mcmc import rminus1
    rng = np.random.default_rng(1)
    for m, n, d in ((4, 50, 1), (8, 200, 3), (32, 100, 5)):
        seqs = rng.normal(size=(m, n, d)) @ rng.normal(size=(d, d)) + rng.normal(0, 0.3, (m, 1, d))
        W = np.mean([np.cov(s, rowvar=False, ddof=1).reshape(d, d) for s in seqs], axis=0)
        B = np.cov(seqs.mean(axis=1), rowvar=False, ddof=1).reshape(d, d)
        direct = np.max(np.abs(np.linalg.eigvals(np.linalg.solve(W, B))))
        assert rminus1(seqs) == pytest.approx(direct, rel=1e-10)


def test_rminus1_of_iid_sequences_is_about_zero():
    from gpry_amd.mcmc import rminus1
    seqs = np.random.default_rng(2).normal(size=(64, 5000, 4))
    assert 0 <= rminus1(seqs) < 0.005
    assert rminus1(seqs[:1]) == np.inf


# ---- the run ------------------------------------------------------------------------------------------------------
def test_adaptation_schedule_and_frozen_proposal():
    from gpry_amd.mcmc import run_mcmc
    from gpry_amd.nested import cholesky_ridged
    d = 3
    ll, bounds = _gauss(d)
    X0, y0 = _training(ll, d)
    dev = Keeper(ll)
    r = run_mcmc(dev, bounds, 5, 16, X0, y0, learn_every=40, learn_batches=3, batch_steps=60, thin=3, max_batches=4,
                 Rminus1_stop=0.0)
    assert [c["nsteps"] for c in dev.calls] == [40] * 3 + [60] * 4
    assert [c["thin"] for c in dev.calls] == [1] * 3 + [3] * 4
    assert [c["batch"] for c in dev.calls] == list(range(7))
    span = bounds[:, 1] - bounds[:, 0]
    scale = 2.38 / np.sqrt(d)
    for k in range(3):
        half = dev.outs[k]["X"][:, 20:].reshape(-1, d)
        C = np.cov((half - bounds[:, 0]) / span, rowvar=False, ddof=0)
        np.testing.assert_allclose(dev.calls[k + 1]["Lp"], scale * cholesky_ridged(C), rtol=1e-12)
    for c in dev.calls[3:]:
        np.testing.assert_array_equal(c["Lp"], dev.calls[3]["Lp"])
    np.testing.assert_allclose(r.covmat, (dev.calls[3]["Lp"] @ dev.calls[3]["Lp"].T) / scale ** 2 * np.outer(span, span),
                               rtol=1e-10)
    assert r.batches == 4 and not r.converged and len(r.Rminus1) == 4


def test_first_proposal_from_covmat_or_the_weighted_training_set():
    from gpry_amd.mcmc import _weighted_cov, run_mcmc
    from gpry_amd.nested import cholesky_ridged
    d = 2
    ll, bounds = _gauss(d)
    X0, y0 = _training(ll, d)
    span = bounds[:, 1] - bounds[:, 0]
    cov = np.array([[0.3, 0.1], [0.1, 0.2]])
    for given, C in ((cov, cov), (None, _weighted_cov(X0, y0))):
        dev = Keeper(ll)
        run_mcmc(dev, bounds, 1, 8, X0, y0, covmat=given, learn_batches=0, batch_steps=10, thin=1, max_batches=1)
        np.testing.assert_allclose(dev.calls[0]["Lp"], 2.38 / np.sqrt(d) * cholesky_ridged(C / np.outer(span, span)),
                                   rtol=1e-12)
    w = np.exp(y0 - y0.max())
    m = w @ X0 / w.sum()
    np.testing.assert_allclose(_weighted_cov(X0, y0), (X0 - m).T @ ((X0 - m) * w[:, None]) / w.sum(), rtol=1e-12)


def test_starts_are_drawn_from_the_training_set_by_weight():
    from gpry_amd.mcmc import run_mcmc
    d = 2
    ll, bounds = _gauss(d)
    X0, y0 = _training(ll, d)
    y0 = y0.copy()
    y0[:10] = -np.inf                      # never a start
    X0[10:20] = 9.0                        # outside the box: never a start
    dev = Keeper(ll)
    seen = {}
    real = dev.mcmc_chains

    def spy(lo, hi, Xs, ys, *a, **k):
        seen.setdefault("X", Xs.copy())
        seen.setdefault("y", ys.copy())
        return real(lo, hi, Xs, ys, *a, **k)

    dev.mcmc_chains = spy
    run_mcmc(dev, bounds, 7, 500, X0, y0, learn_batches=0, batch_steps=2, thin=1, max_batches=1)
    ok = np.arange(20, len(y0))
    p = np.exp(y0[ok] - y0[ok].max())
    expect = X0[ok][np.random.default_rng(7).choice(len(ok), size=500, p=p / p.sum())]
    np.testing.assert_array_equal(seen["X"], expect)
    assert np.all(np.isnan(seen["y"]))                  # evaluated by the device
    assert np.all(dev.outs[0]["ncalls"] >= 1)


def test_stops_on_rminus1():
    from gpry_amd.mcmc import run_mcmc
    ll, bounds = _gauss(2)
    X0, y0 = _training(ll, 2)
    r = run_mcmc(Keeper(ll), bounds, 1, 64, X0, y0, batch_steps=100, Rminus1_stop=0.02)
    assert r.converged and r.Rminus1[-1] < 0.02 and np.all(r.Rminus1[:-1] >= 0.02)
    assert 0.1 < r.acceptance < 0.8
    np.testing.assert_allclose(np.average(r.X, weights=r.w, axis=0), 0.3, atol=0.05)


def test_stops_on_max_ncalls_and_max_batches():
    from gpry_amd.mcmc import run_mcmc
    ll, bounds = _gauss(2)
    X0, y0 = _training(ll, 2)
    dev = Keeper(ll)
    cap = 16 * (4 * 50 + 3 * 40)
    r = run_mcmc(dev, bounds, 1, 16, X0, y0, learn_every=50, batch_steps=40, Rminus1_stop=0.0, max_ncalls=cap)
    assert not r.converged and r.ncalls >= cap
    assert r.ncalls - int(np.sum(dev.outs[-1]["ncalls"])) < cap
    assert r.ncalls == sum(int(np.sum(o["ncalls"])) for o in dev.outs)
    r = run_mcmc(Keeper(ll), bounds, 1, 16, X0, y0, batch_steps=40, Rminus1_stop=0.0, max_batches=3)
    assert not r.converged and r.batches == 3 and len(r.Rminus1) == 3


def test_skip_fraction_and_temperature_weights():
    from gpry_amd.mcmc import run_mcmc
    d = 2
    ll, bounds = _gauss(d)
    X0, y0 = _training(ll, d)
    for T, reset in ((1.0, True), (2.0, True), (2.0, False)):
        dev = Keeper(ll)
        r = run_mcmc(dev, bounds, 3, 8, X0, y0, learn_batches=1, learn_every=20, batch_steps=30, thin=2, max_batches=3,
                     Rminus1_stop=0.0, skip=0.4, temperature=T, reset_temperature=reset)
        assert all(c["T"] == T for c in dev.calls)
        recX = np.concatenate([o["X"] for o in dev.outs[1:]], axis=1)
        recy = np.concatenate([o["y"] for o in dev.outs[1:]], axis=1)
        first = int(0.4 * recX.shape[1])
        assert recX.shape[1] == 45 and first == 18
        np.testing.assert_array_equal(r.X, recX[:, first:].reshape(-1, d))
        np.testing.assert_array_equal(r.y, recy[:, first:].ravel())
        if T != 1.0 and reset:
            lw = r.y - r.y / T
            np.testing.assert_allclose(r.w, np.exp(lw - lw.max()) / np.sum(np.exp(lw - lw.max())), rtol=1e-12)
        else:
            np.testing.assert_array_equal(r.w, np.full(len(r.y), 1.0 / len(r.y)))
        assert abs(np.sum(r.w) - 1) < 1e-12


def test_run_mcmc_argument_errors():
    from gpry_amd.mcmc import run_mcmc
    ll, bounds = _gauss(2)
    X0, y0 = _training(ll, 2)
    dev = Keeper(ll)
    for kw, msg in ((dict(nchains=0), "nchains"), (dict(temperature=0.0), "temperature"),
                    (dict(temperature=np.inf), "temperature"), (dict(thin=50, batch_steps=10), "thin"),
                    (dict(learn_every=1), "learn_every"), (dict(skip=1.0), "skip"), (dict(max_batches=0), "max_batches")):
        args = dict(nchains=4)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            run_mcmc(dev, bounds, 1, args.pop("nchains"), X0, y0, **args)
    with pytest.raises(ValueError, match="finite"):
        run_mcmc(dev, bounds, 1, 4, X0, np.full(len(y0), -np.inf))
    with pytest.raises(ValueError, match="dimension"):
        run_mcmc(dev, bounds, 1, 4, X0[:, :1], y0)
    assert dev.calls == []


# ---- the public calls, on a stand-in model ---------------------------------------------------------------------------
class FakeDevice(mcmc_numpy.NumpyMCMCDevice):
    def __init__(self, loglike):
        super().__init__(loglike)
        self.ns = ns_philox.NumpyNestedDevice(loglike)
        self.ns_prior, self.ns_generation = self.ns.ns_prior, self.ns.ns_generation


class FakeGPR:
    minus_inf_value = -np.inf

    def __init__(self, d=2, gates=True, trust_bounds=None):
        self.loglike, self.bounds = _gauss(d)
        self.X_train, self.y_train = _training(self.loglike, d)
        self.trust_bounds = trust_bounds
        self.device = FakeDevice(self.loglike)
        self.gates, self.pushes, self.n_eval = gates, [], 0

    def _ensure_factor(self):
        self.pushes.append("factor")

    def _push_affine(self):
        self.pushes.append("affine")

    def _push_gates(self, ignore_trust_region=False, sinks=None):
        self.pushes.append("gates")
        return self.gates


def test_nested_options_and_xnumbers():
    from gpry_amd.mc import nested_settings
    assert nested_settings(3) == dict(nlive=75, num_repeats=15, precision_criterion=0.001, nprior=75, max_ncalls=None)
    s = nested_settings(4, {"nlive": "50d", "num_repeats": 7, "nprior": "2d2", "max_ncalls": "1000d"})
    assert s == dict(nlive=200, num_repeats=7, precision_criterion=0.001, nprior=32, max_ncalls=4000)
    with pytest.warns(UserWarning, match="do_clustering"):
        assert nested_settings(2, {"do_clustering": True})["nlive"] == 50
    with pytest.raises(ValueError, match="nlive"):
        nested_settings(2, {"nlive": "lots"})


def test_mcmc_options_cobaya_names_and_warnings():
    from gpry_amd.mc import mcmc_settings
    s = mcmc_settings(3, {"Rminus1_stop": 0.05, "temperature": 2, "max_samples": "1000d", "nchains": 64,
                          "covmat": np.eye(3)})
    assert s["Rminus1_stop"] == 0.05 and s["temperature"] == 2 and s["max_ncalls"] == 3000 and s["nchains"] == 64
    np.testing.assert_array_equal(s["covmat"], np.eye(3))
    with pytest.warns(UserWarning, match="Rminus1_cl_stop"):
        s = mcmc_settings(3, {"Rminus1_cl_stop": 0.2, "Rminus1_stop": 0.02})
    assert s == {"Rminus1_stop": 0.02}


def test_mc_sample_from_gp_both_samplers_and_the_output_file(tmp_path):
    from gpry_amd.mc import mc_sample_from_gp
    from gpry_amd.nested import run_nested
    gpr = FakeGPR()
    X, y, w = mc_sample_from_gp(gpr, sampler="nested", sampler_options={"nlive": "10d"}, seed=4,
                                output=str(tmp_path / "out" / "ns"))
    assert gpr.pushes == ["factor", "affine", "gates"]
    r = run_nested(ns_philox.NumpyNestedDevice(gpr.loglike), gpr.bounds, 4, 20, 10, precision_criterion=0.001, nprior=20)
    np.testing.assert_array_equal(X, r.X)
    np.testing.assert_array_equal(w, r.w)
    assert gpr.n_eval == r.ncalls
    path = tmp_path / "out" / "ns.txt"
    assert open(path).readline().strip() == "# w minuslogp x_1 x_2"
    table = np.loadtxt(path)
    np.testing.assert_allclose(table, np.column_stack([w, -y, X]), rtol=1e-15)
    X, y, w = mc_sample_from_gp(gpr, sampler="MCMC", sampler_options={"nchains": 32, "Rminus1_stop": 0.05}, seed=2,
                                output=str(tmp_path / "chain.dat"))
    res = mc_sample_from_gp.last_result
    assert res.converged and res.Rminus1[-1] < 0.05 and len(X) == len(y) == len(w)
    assert gpr.device.calls[0]["nchains"] == 32
    np.testing.assert_allclose(np.loadtxt(tmp_path / "chain.dat"), np.column_stack([w, -y, X]), rtol=1e-15)


def test_default_bounds_are_the_trust_region():
    from gpry_amd.mc import mc_sample_from_gp
    tb = np.array([[-1.0, 2.0], [-0.5, 1.0]])
    gpr = FakeGPR(trust_bounds=tb)
    X, _, _ = mc_sample_from_gp(gpr, sampler="mcmc", sampler_options={"nchains": 8, "max_batches": 2}, seed=1)
    assert np.all((X >= tb[:, 0]) & (X <= tb[:, 1]))
    gpr = FakeGPR()
    mc_sample_from_gp(gpr, sampler="mcmc", sampler_options={"nchains": 8, "max_batches": 1}, seed=1)
    assert gpr.device.calls


def test_public_call_errors():
    from gpry_amd.mc import mc_sample_from_gp, mc_sample_from_gp_ns
    with pytest.raises(ValueError, match="sampler"):
        mc_sample_from_gp(FakeGPR(), sampler="polychord")
    for s in ("nested", "mcmc"):
        with pytest.raises(ValueError, match="no device form"):
            mc_sample_from_gp(FakeGPR(gates=False), sampler=s, seed=1)
    with pytest.raises(ValueError, match="run=True"):
        mc_sample_from_gp_ns(FakeGPR(), run=False)
    with pytest.raises(ValueError, match="unknown"):
        mc_sample_from_gp_ns(FakeGPR(), sampler="multinest")


def test_small_chain_proposer_falls_back_to_uniform_points():
    from gpry_amd.proposal import SmallChainProposer
    gpr = FakeGPR()
    gpr.device.loglike = lambda X: np.full(len(np.atleast_2d(X)), -np.inf)    # nothing is ever accepted
    p = SmallChainProposer(gpr.bounds, npoints=30, nsteps=5, nretries=2)
    with pytest.raises(ValueError, match="update"):
        p.get(rng=np.random.default_rng(0))
    p.update(gpr)
    pts = np.array([p.get(rng=np.random.default_rng(1)) for _ in range(5)])
    assert len(gpr.device.calls) == 2 and all(c["nsteps"] == 30 and c["nchains"] == 1 for c in gpr.device.calls)
    assert np.all((pts >= gpr.bounds[:, 0]) & (pts <= gpr.bounds[:, 1]))


def test_small_chain_proposer_hands_out_the_chain_from_its_end():
    from gpry_amd.proposal import SmallChainProposer
    gpr = FakeGPR()
    p = SmallChainProposer(gpr.bounds, npoints=100, nsteps=20)
    p.update(gpr)
    keep = Keeper(gpr.loglike)
    gpr.device = keep
    pts = np.array([p.get(rng=np.random.default_rng(3)) for _ in range(5)])
    assert len(keep.calls) == 1
    np.testing.assert_array_equal(pts, keep.outs[0]["X"][0][::-20][::-1])
    rng = np.random.default_rng(3)
    i = rng.choice(range(len(gpr.X_train)))
    assert keep.calls[0]["nchains"] == 1
    assert np.array_equal(keep.outs[0]["X"][0][0], gpr.X_train[i]) or keep.outs[0]["naccept"][0] > 0


def test_patch_gpry_mc_puts_the_device_sampler_under_the_runner(monkeypatch):
    from gpry_amd import mc as dmc
    from gpry_amd.integration import patch_gpry_mc
    pkg = types.ModuleType("gpry")
    mc = types.ModuleType("gpry.mc")

    def cpu_sampler(*a, **k):
        raise AssertionError("the reference's sampler ran")

    mc.mc_sample_from_gp_ns = cpu_sampler
    run = types.ModuleType("gpry.run")
    run.mc = mc

    class Runner:
        """generate_mc_sample's "nested" branch (gpry/run.py:1655-1681)."""

        def __init__(self, gpr):
            self.gpr, self.d = gpr, gpr.bounds.shape[0]

        def generate_mc_sample(self, output=None):
            return run.mc.mc_sample_from_gp_ns(self.gpr, bounds=None, params=["a", "b"], sampler=None,
                                               sampler_options={"nlive": 50 * self.d}, output=output, verbose=3)

    run.Runner = Runner
    pkg.mc, pkg.run = mc, run
    for name, mod in (("gpry", pkg), ("gpry.mc", mc), ("gpry.run", run)):
        monkeypatch.setitem(sys.modules, name, mod)
    assert patch_gpry_mc() is mc
    assert mc.mc_sample_from_gp_ns is dmc.mc_sample_from_gp_ns
    gpr = FakeGPR()
    X, y, w = Runner(gpr).generate_mc_sample()
    assert gpr.pushes == ["factor", "affine", "gates"] and len(X) > 100 and abs(np.sum(w) - 1) < 1e-12
    assert gpr.device.ns.calls and gpr.device.calls == []


def test_rminus1_from_batch_sums_equals_the_direct_form():
    from gpry_amd.mcmc import _Records, rminus1
    rng = np.random.default_rng(4)
    rec = _Records()
    for n in (7, 12, 30, 5):
        rec.add(rng.normal(size=(6, n, 3)) + 2.0, rng.normal(size=(6, n)))
        for first in (0, 3, int(0.33 * rec.n)):
            allX = np.concatenate(rec.X, axis=1)[:, first:]
            h = allX.shape[1] // 2
            direct = rminus1(np.concatenate([allX[:, :h], allX[:, h:2 * h]])) if h >= 2 else np.inf
            assert rec.rminus1(first) == pytest.approx(direct, rel=1e-9)


def test_the_entry_point_refuses_a_null_context():
    from gpry_amd import _lib
    lib = _lib.load_library()
    z = np.zeros(4)
    rc = lib.gpry_mcmc_chains(None, _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), 1, _lib._ptr(z), 1.0,
                              -np.inf, 0, 0, 1, 1, None, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"ctx is NULL" in lib.gpry_last_error(None)
