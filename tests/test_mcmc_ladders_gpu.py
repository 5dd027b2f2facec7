"""The tempered Metropolis ladders on the device (gpry_amd/csrc/mcmc_ladders.hip, gpry_mcmc_ladders; gpry_amd/tempering.py,
gpry_amd/mc.py): every recorded, final and proposed y equals gpr.predict of its row bit for bit (the model cases of
test_nested_gpu.py); with swaps off every slot is the plain chain of gpry_mcmc_chains bit for bit, at every DP bucket,
kernel id and ladder size; every Metropolis and swap decision follows the rule restated with the numpy Philox draws; the
same seed gives the same bits on two contexts and whatever the number of ladders; the cold rung crosses between two
separated modes, which the plain kernel cannot, and finds their masses; every rung samples its own temperature;
mc_sample_from_gp runs it; the entry point's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import gpry_oracle as orc
from test_host_mirror_gpu import make_gpr
from test_mcmc_gpu import _moment_target, _moments, _proposal, _pushed, _starts
from test_nested_gpu import _fixed, _gauss_ll, _one_point, _parity_cases, _quadrature

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ladder_walk  # noqa: E402
import sampler_walk as sw  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("X", "y", "X_last", "y_last", "naccept", "ncalls")


def _ladder_proposals(gpr, bounds, T, scale=1.0):
    """The weighted training covariance's factor, widened by sqrt(T[r] / T[0]) per rung."""
    L = _proposal(gpr, bounds, scale)
    return np.array([L * np.sqrt(t / T[0]) for t in T])


# ---- 1. parity of y --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrungs", [2, 3, 8])
@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()])
def test_every_recorded_and_proposed_y_equals_one_point_predict(case, nrungs):
    gpr, bounds = dict(_parity_cases())[case]()
    _pushed(gpr)
    d, n, steps = len(bounds), 3 * nrungs, 40
    T = 1.6 ** np.arange(nrungs)
    X0 = _starts(gpr, n, 3)
    out = gpr.device.mcmc_ladders(bounds[:, 0], bounds[:, 1], X0, np.full(n, np.nan), nrungs,
                                  _ladder_proposals(gpr, bounds, T), T, gpr.minus_inf_value, 77, 0, steps, 2, 4,
                                  proposals=True)
    Xr, yr = out["X"].reshape(-1, d), out["y"].ravel()
    np.testing.assert_array_equal(yr, _one_point(gpr, Xr))
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, out["X_last"]))
    ev = ~np.isnan(out["y_prop"].ravel())
    Xp = out["X_prop"].reshape(-1, d)[ev]
    np.testing.assert_array_equal(out["y_prop"].ravel()[ev], _one_point(gpr, Xp))
    assert np.all(np.isfinite(yr)) and np.all((Xr >= bounds[:, 0]) & (Xr <= bounds[:, 1]))
    # the start's evaluation and one per evaluated proposal
    np.testing.assert_array_equal(out["ncalls"], 1 + np.sum(~np.isnan(out["y_prop"]), axis=1))
    assert np.sum(out["naccept"]) > 0 and out["swap_log"].shape == (3, 10, nrungs - 1)
    assert np.sum(out["nswap_try"]) > 0
    if case == "SVM + trust region":
        assert np.any(np.isneginf(out["y_prop"])), "no proposal met the gates"
        assert np.all(gpr.predict(Xr) > -np.inf)


# ---- 2. swaps off: the plain chains ----------------------------------------------------------------------------------
def _equals_plain_chains(gpr, bounds, nrungs, nladders=3, steps=30, thin=2, seed=41, batch=3):
    _pushed(gpr)
    n = nladders * nrungs
    lo, hi = bounds[:, 0], bounds[:, 1]
    T = 1.0 + 0.7 * np.arange(nrungs)
    Lp = _ladder_proposals(gpr, bounds, T)
    X0 = _starts(gpr, n, 5)
    y0 = np.full(n, np.nan)
    y0[1::2] = _one_point(gpr, X0[1::2])            # (a given y0 is taken as it is)
    out = gpr.device.mcmc_ladders(lo, hi, X0, y0, nrungs, Lp, T, gpr.minus_inf_value, seed, batch, steps, thin, 0,
                                  proposals=True)
    assert not out["nswap_try"].any() and out["swap_log"].size == 0
    for r in range(nrungs):
        ref = gpr.device.mcmc_chains(lo, hi, X0, y0, Lp[r], T[r], gpr.minus_inf_value, seed, batch, steps, thin,
                                     proposals=True)
        for k in KEYS + ("X_prop", "y_prop"):
            np.testing.assert_array_equal(out[k][r::nrungs], ref[k][r::nrungs], err_msg=f"slot {r}: {k}")
    assert out["naccept"].sum() > 0
    return out


# (d, kernel id) -> nrungs: every DP bucket x kernel id once, the three RP buckets spread over them
_BUCKET_CASES = [(d, kid, (2, 4, 8)[(i + kid) % 3]) for i, d in enumerate((3, 7, 13, 20)) for kid in range(4)]


@pytest.mark.parametrize("d,kid,nrungs", _BUCKET_CASES)
def test_without_swaps_every_slot_is_the_plain_chain(d, kid, nrungs):
    m = sw.Model(d, kid, 200)
    _equals_plain_chains(m.gpr(), m.bounds, nrungs)


@pytest.mark.parametrize("case", [c[0] for c in _parity_cases()][:3])
def test_without_swaps_every_slot_is_the_plain_chain_at_every_nsplit(case):
    gpr, bounds = dict(_parity_cases())[case]()
    _equals_plain_chains(gpr, bounds, 3)


def test_one_rung_is_the_plain_kernel():
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _equals_plain_chains(gpr, bounds, 1, nladders=8)


# ---- 3. the rule, step by step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,swap_every,thin", [([1.0, 2.0, 4.0], 1, 1), ([1.0, 1.5, 2.25, 3.4, 5.0], 3, 2)])
def test_every_step_and_every_swap_follows_the_rule(T, swap_every, thin):
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    T = np.array(T)
    R, nl, steps = len(T), 8, 60
    X0 = _starts(gpr, nl * R, 4)
    counts = ladder_walk.check_ladder_rule(gpr.device, bounds[:, 0], bounds[:, 1], X0, np.full(nl * R, np.nan),
                                           _one_point(gpr, X0), R, _ladder_proposals(gpr, bounds, T), T,
                                           gpr.minus_inf_value, 1234, 5, steps, thin, swap_every)
    assert counts["parities"] == {0, 1}
    assert counts["swaps_accepted"] > 0 and counts["swaps_rejected"] > 0 and counts["accepted"] > 0


# ---- 4. the same bits ------------------------------------------------------------------------------------------------
def test_same_seed_same_bits_on_two_contexts_and_any_number_of_ladders():
    theta = np.log([4.0, 0.3, 0.3, 0.3, 0.3])
    gpr, bounds = _fixed(_gauss_ll(4), 4, 1500, theta)
    gpr2, _ = _fixed(_gauss_ll(4), 4, 1500, theta)
    assert gpr2.device is not gpr.device
    R = 4
    T = 2.0 ** np.arange(R)
    Lp = _ladder_proposals(_pushed(gpr), bounds, T)
    _pushed(gpr2)
    X0 = _starts(gpr, 16 * R, 8)
    args = (bounds[:, 0], bounds[:, 1])
    a = gpr.device.mcmc_ladders(*args, X0, np.full(16 * R, np.nan), R, Lp, T, -np.inf, 9, 2, 50, 1, 2)
    b = gpr2.device.mcmc_ladders(*args, X0, np.full(16 * R, np.nan), R, Lp, T, -np.inf, 9, 2, 50, 1, 2)
    e = gpr.device.mcmc_ladders(*args, X0[:2 * R], np.full(2 * R, np.nan), R, Lp, T, -np.inf, 9, 2, 50, 1, 2)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][:2 * R], e[k])
    for k in ("nswap_try", "nswap_acc"):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][:2], e[k])
    assert a["nswap_acc"].sum() > 0
    f = gpr.device.mcmc_ladders(*args, X0, np.full(16 * R, np.nan), R, Lp, T, -np.inf, 10, 2, 50, 1, 2)
    assert not np.array_equal(a["X"], f["X"])


# ---- 5. two separated modes ------------------------------------------------------------------------------------------
_S, _A, _B = 0.24, np.array([-1.6, -1.6]), np.array([1.28, 1.28])


def _mixture_ll(X):
    X = np.atleast_2d(X)
    return np.logaddexp(np.log(0.7) - 0.5 * np.sum((X - _A) ** 2, axis=1) / _S ** 2,
                        np.log(0.3) - 0.5 * np.sum((X - _B) ** 2, axis=1) / _S ** 2)


def _mixture_model():
    """The surrogate fitted to the mixture in [-4, 4]^2: 100 points around each mode (sigma 2 s), 100 uniform ones."""
    rng = np.random.default_rng(0)
    bounds = np.array([[-4.0, 4.0]] * 2)
    X = np.concatenate([rng.normal(_A, 2 * _S, (100, 2)), rng.normal(_B, 2 * _S, (100, 2)),
                        rng.uniform(-4, 4, (100, 2))]).clip(-4, 4)
    gpr = make_gpr(bounds, orc.MATERN52, n_restarts_optimizer=1, random_state=1)
    gpr.append_to_data(X, _mixture_ll(X), fit_gpr=True)
    return gpr, bounds


def _mode_1(X):
    return np.sum(X, axis=-1) < -0.32


def _grid_mass(gpr, bounds, n):
    ax = [bounds[k, 0] + (np.arange(n) + 0.5) * (bounds[k, 1] - bounds[k, 0]) / n for k in range(2)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 2)
    y = gpr.predict(G)
    p = np.exp(y - np.max(y))
    return float(p[_mode_1(G)].sum() / p.sum())


def test_the_cold_rung_crosses_between_modes_where_the_plain_kernel_cannot():
    from gpry_amd.mcmc import _starts as draw_starts
    gpr, bounds = _mixture_model()
    m200, m400 = _grid_mass(gpr, bounds, 200), _grid_mass(gpr, bounds, 400)
    _pushed(gpr)
    lo, hi = bounds[:, 0], bounds[:, 1]
    nl, R, steps = 64, 6, 3000
    T = 36.0 ** (np.arange(R) / (R - 1))
    Lp = np.array([2.38 / np.sqrt(2) * _S / 8 * np.sqrt(t) * np.eye(2) for t in T])
    Xs, ys = draw_starts(gpr.X_train, gpr.y_train, lo, hi, 1.0, gpr.minus_inf_value, nl * R, 7)[2:]
    out = gpr.device.mcmc_ladders(lo, hi, Xs, ys, R, Lp, T, gpr.minus_inf_value, 7, 0, steps, 5, 5)
    side = _mode_1(out["X"][0::R])
    crossings = int(np.sum(side[:, 1:] != side[:, :-1]))
    frac = side[:, side.shape[1] // 3:].mean(axis=1)
    se = frac.std(ddof=1) / np.sqrt(nl)
    swap = out["nswap_acc"].sum(axis=0) / np.maximum(out["nswap_try"].sum(axis=0), 1)
    print(f"crossings {crossings}, mass of mode 1 {frac.mean():.4f} (SE {se:.4f}), quadrature {m400:.6f} (n = 200: "
          f"{m200:.6f}), swap acceptance {np.round(swap, 3)}, device {out['device_ms']:.1f} ms")
    assert crossings >= 1
    plain = gpr.device.mcmc_chains(lo, hi, Xs[0::R], ys[0::R], Lp[0], 1.0, gpr.minus_inf_value, 7, 0, steps, 5)
    ps = _mode_1(plain["X"])
    assert np.sum(ps[:, 1:] != ps[:, :-1]) == 0
    assert plain["naccept"].sum() > 0.1 * nl * steps
    assert abs(frac.mean() - m400) <= 4 * se + abs(m400 - m200), (frac.mean(), m400, se)


# ---- 6. every rung has its own distribution --------------------------------------------------------------------------
class _Recorder:
    def __init__(self, dev):
        self.dev, self.outs = dev, []

    def mcmc_ladders(self, *a, **k):
        self.outs.append(self.dev.mcmc_ladders(*a, **k))
        return self.outs[-1]


@pytest.fixture(scope="module")
def gauss2():
    gpr, bounds, n = _moment_target("gauss d=2")
    _, mq, Cq = _quadrature(gpr, bounds, n)
    return gpr, bounds, mq, Cq


def test_every_rung_has_its_own_distribution(gauss2):
    from gpry_amd.tempering import run_tempered
    gpr, bounds, mq, Cq = gauss2
    sd = np.sqrt(np.diag(Cq))
    _pushed(gpr)
    rec = _Recorder(gpr.device)
    r = run_tempered(rec, bounds, 4, 64, gpr.X_train, gpr.y_train, temperatures=[1.0, 2.0, 4.0],
                     minus_inf_value=gpr.minus_inf_value)
    print(f"batches {r.batches}, R - 1 {r.Rminus1[-1]:.4f}, acceptance per rung {np.round(r.acceptance_per_rung, 3)}, swap "
          f"acceptance {np.round(r.swap_acceptance, 3)}, ncalls {r.ncalls}, device {r.device_s:.2f} s")
    assert r.converged and r.Rminus1[-1] < 0.01
    m, Cv = _moments(r.X, r.w)
    assert np.all(np.abs(m - mq) < 0.1 * sd), (m, mq, sd)
    assert np.all(np.abs(Cv - Cq) <= 0.2 * np.outer(sd, sd)), (Cv, Cq)
    np.testing.assert_array_equal(r.y[:200], _one_point(gpr, r.X[:200]))
    # the rung at T = 2, from the sampling batches' records without the burn-in
    warm = np.concatenate([o["X"][1::3] for o in rec.outs[4:]], axis=1)
    warm = warm[:, int(0.33 * warm.shape[1]):].reshape(-1, 2)
    _, C2 = _moments(warm, np.full(len(warm), 1.0 / len(warm)))
    assert np.all(np.abs(C2 - 2 * Cq) <= 0.4 * np.outer(sd, sd)), (C2, 2 * Cq)


# ---- 7. the public call ----------------------------------------------------------------------------------------------
def test_mc_sample_from_gp_tempered(gauss2):
    from gpry_amd.mc import mc_sample_from_gp
    gpr, bounds = gauss2[:2]
    before = mc_sample_from_gp(gpr, bounds=bounds, sampler="mcmc", seed=22, sampler_options={"nchains": 32, "max_batches": 2})
    n0 = gpr.n_eval
    opts = {"nchains": 16, "rungs": 3, "max_batches": 2, "batch_steps": 200}
    X, y, w = mc_sample_from_gp(gpr, bounds=bounds, sampler="tempered", seed=23, sampler_options=opts)
    res, n1 = mc_sample_from_gp.last_result, gpr.n_eval
    assert len(res.temperatures) == 3 and res.batches <= 2
    assert w.sum() == pytest.approx(1.0) and np.all(w >= 0) and len(X) == len(y) == len(w) > 0
    np.testing.assert_array_equal(y[:200], _one_point(gpr, X[:200]))
    assert n1 - n0 == res.ncalls > 16 * 3 * 400
    with pytest.warns(UserWarning, match="eps"):
        mc_sample_from_gp(gpr, bounds=bounds, sampler="tempered", seed=23, sampler_options={**opts, "eps": 0.1})
    after = mc_sample_from_gp(gpr, bounds=bounds, sampler="mcmc", seed=22, sampler_options={"nchains": 32, "max_batches": 2})
    for u, v in zip(before, after):
        np.testing.assert_array_equal(u, v)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_before_anything_runs():
    from gpry_amd._lib import GpryHipError, _ptr
    gpr, bounds = dict(_parity_cases())["N=600 d=3 (nsplit 1)"]()
    _pushed(gpr)
    dev = gpr.device
    d, R, nl = 3, 2, 2
    lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])

    def call(nladders=nl, nrungs=R, T=(1.0, 2.0), swap_every=1, nsteps=4, thin=1, batch=0, log=False, lo=lo, hi=hi,
             y_prop=True):
        n = nl * 8
        X0, y0 = np.full((n, d), 0.3), np.full(n, np.nan)
        Lp, T = np.tile(0.05 * np.eye(d), (8, 1, 1)), np.array(list(T) + [1.0] * 8)
        o = dict(X=np.zeros((n, 4, d)), y=np.zeros((n, 4)), Xl=np.zeros((n, d)), yl=np.zeros(n), na=np.zeros(n, np.int64),
                 nc=np.full(n, -7, np.int64), nt=np.zeros((nl, 7), np.int64), ns=np.zeros((nl, 7), np.int64),
                 Xp=np.zeros((n, 4, d)), yp=np.zeros((n, 4)), lg=np.zeros((nl, 4, 7), np.int8))
        rc = dev._lib.gpry_mcmc_ladders(dev._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), int(nladders), int(nrungs), _ptr(Lp),
                                        _ptr(T), -np.inf, 1, int(batch), int(nsteps), int(thin), int(swap_every),
                                        _ptr(o["X"]), _ptr(o["y"]), _ptr(o["Xl"]), _ptr(o["yl"]), _ptr(o["na"]),
                                        _ptr(o["nc"]), _ptr(o["nt"]), _ptr(o["ns"]), _ptr(o["Xp"]),
                                        _ptr(o["yp"]) if y_prop else None, _ptr(o["lg"]) if log else None,
                                        C.byref(C.c_double(0.0)))
        assert rc == 0 or np.all(o["nc"] == -7), "a refused call wrote its outputs"
        dev._check(rc, "gpry_mcmc_ladders")
        return o

    assert np.all(call(log=True)["nc"][:nl * R] >= 1)
    for kw, msg in ((dict(nrungs=0), "nrungs"), (dict(nrungs=9), "nrungs"), (dict(T=(1.0, 0.0)), "temperature"),
                    (dict(T=(1.0, -2.0)), "temperature"), (dict(T=(np.inf, 2.0)), "temperature"),
                    (dict(T=(1.0, np.nan)), "temperature"), (dict(swap_every=-1), "swap_every"),
                    (dict(nladders=2 ** 28, nrungs=8), "nladders"), (dict(swap_every=0, log=True), "swap_log"),
                    (dict(nladders=0), "nladders"), (dict(nsteps=-1), "nsteps"), (dict(thin=0), "thin"),
                    (dict(batch=-1), "batch"), (dict(batch=2 ** 32), "batch"), (dict(y_prop=False), "X_prop"),
                    (dict(hi=lo), "bounds")):
        with pytest.raises(GpryHipError, match=msg):
            call(**kw)
    with pytest.raises(GpryHipError, match="nrungs"):
        dev.mcmc_ladders(lo, hi, np.full((9, d), 0.3), np.full(9, np.nan), 9, np.tile(np.eye(d), (9, 1, 1)), np.ones(9),
                         -np.inf, 1, 0, 2, 1, 0)
