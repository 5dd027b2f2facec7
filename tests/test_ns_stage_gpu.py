"""The staged call buffer behind the sampler and optimiser entry points (NsStage of gpry_amd/csrc/ns_common.h): its two
backings give the same bits; a region that is empty -- no steps, no records, one rung, no points, no iterations -- comes
back as an empty array beside outputs that equal what is stated for them here; the test hooks' regions leave every other
output as it is without them.  One small model (48 rows, d = 3: one mean slice) serves every test: nothing here
depends on the shapes, the entry points' own suites cover those."""
import numpy as np
import pytest

from test_mcmc_gpu import _proposal, _pushed
from test_nested_gpu import _fitted, _gauss_ll, _one_point

pytestmark = pytest.mark.gpu

D = 3
_MODEL = []


def _model():
    """(gpr, lo, hi, Lp, X0): the fitted model, its box, a proposal factor and four starts inside the box."""
    if not _MODEL:
        gpr, bounds = _fitted(_gauss_ll(D), D, 48)
        _pushed(gpr)
        lo, hi = bounds[:, 0], bounds[:, 1]
        X0 = np.random.default_rng(5).uniform(-1.0, 1.0, (4, D))
        _MODEL.append((gpr, lo, hi, _proposal(gpr, bounds), X0))
    return _MODEL[0]


def _nan(n):
    return np.full(n, np.nan)


def _assert_same(a, b, keys=None):
    """The arrays of two output dicts are equal bit for bit (NaN equal to NaN); without ``keys``: all but device_ms."""
    if keys is None:
        assert a.keys() == b.keys()
        keys = [k for k in a if k != "device_ms"]
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- the two backings -------------------------------------------------------------------------------------------------
def _both_backings(dev, call):
    outs = []
    try:
        for mapped in (0, 1):
            dev.set_option("mcmc_mapped", mapped)
            outs.append(call())
    finally:
        dev.set_option("mcmc_mapped", 0)
    return outs


def test_mcmc_chains_mapped_and_device_backing_agree_bit_for_bit():
    gpr, lo, hi, Lp, X0 = _model()
    a, b = _both_backings(gpr.device, lambda: gpr.device.mcmc_chains(lo, hi, X0, _nan(4), Lp, 1.0, gpr.minus_inf_value, 11, 3,
                                                                     6, 2, proposals=True))
    assert a["X"].shape == (4, 3, D) and a["X_prop"].shape == (4, 6, D) and np.all(a["ncalls"] >= 1)
    _assert_same(a, b)


def test_mcmc_ladders_mapped_and_device_backing_agree_bit_for_bit():
    gpr, lo, hi, Lp, X0 = _model()
    X6 = np.concatenate([X0, 0.5 * X0[:2]])
    Lps, T = np.stack([Lp, 1.5 * Lp, 2.0 * Lp]), np.array([1.0, 2.0, 4.0])
    a, b = _both_backings(gpr.device, lambda: gpr.device.mcmc_ladders(lo, hi, X6, _nan(6), 3, Lps, T, gpr.minus_inf_value, 11,
                                                                      3, 6, 2, 2, proposals=True))
    assert a["X"].shape == (6, 3, D) and a["nswap_try"].shape == (2, 2) and a["swap_log"].shape == (2, 3, 2)
    _assert_same(a, b)


# ---- empty regions ----------------------------------------------------------------------------------------------------
def _chains(kind, dev, lo, hi, X0, Lp, nsteps, thin, seed=7):
    if kind == "mcmc":
        return dev.mcmc_chains(lo, hi, X0, _nan(len(X0)), Lp, 1.0, -np.inf, seed, 0, nsteps, thin)
    return dev.hmc_chains(lo, hi, X0, _nan(len(X0)), Lp, 0.1, 2, 1.0, -np.inf, seed, 0, nsteps, thin)


@pytest.mark.parametrize("kind", ["mcmc", "hmc"])
def test_no_steps_returns_the_evaluated_starts_and_an_empty_record(kind):
    gpr, lo, hi, Lp, X0 = _model()
    out = _chains(kind, gpr.device, lo, hi, X0, Lp, 0, 1)
    np.testing.assert_array_equal(out["X_last"], X0)
    np.testing.assert_array_equal(out["y_last"], _one_point(gpr, X0))
    np.testing.assert_array_equal(out["ncalls"], 1)
    np.testing.assert_array_equal(out["naccept"], 0)
    assert out["X"].shape == (4, 0, D) and out["y"].shape == (4, 0)


@pytest.mark.parametrize("kind", ["mcmc", "hmc"])
def test_thin_above_nsteps_records_nothing_and_ends_where_thin_one_ends(kind):
    gpr, lo, hi, Lp, X0 = _model()
    out = _chains(kind, gpr.device, lo, hi, X0, Lp, 5, 6)
    every = _chains(kind, gpr.device, lo, hi, X0, Lp, 5, 1)
    assert out["X"].shape == (4, 0, D) and out["y"].shape == (4, 0)
    assert every["X"].shape == (4, 5, D)
    np.testing.assert_array_equal(out["X_last"], every["X"][:, -1])
    np.testing.assert_array_equal(out["y_last"], every["y"][:, -1])
    _assert_same(out, every, ["naccept", "ncalls"])


def test_one_rung_has_no_swap_arrays_and_equals_the_plain_chains():
    gpr, lo, hi, Lp, X0 = _model()
    dev, args = gpr.device, (gpr.minus_inf_value, 21, 2, 6, 2)
    lad = dev.mcmc_ladders(lo, hi, X0, _nan(4), 1, Lp[None], np.array([1.5]), *args, 2, proposals=True)
    one = dev.mcmc_chains(lo, hi, X0, _nan(4), Lp, 1.5, *args, proposals=True)
    assert lad["nswap_try"].shape == (4, 0) and lad["nswap_acc"].shape == (4, 0) and lad["swap_log"].shape == (4, 3, 0)
    assert np.sum(lad["naccept"]) > 0
    _assert_same(lad, one, [k for k in one if k != "device_ms"])


def test_no_points_and_no_chains_return_empty_arrays():
    gpr, lo, hi, Lp, X0 = _model()
    X, y, _ = gpr.device.ns_prior(lo, hi, 3, 0)
    assert X.shape == (0, D) and y.shape == (0,)
    Xs, ys, _ = gpr.device.ns_prior(lo, hi, 3, 8)
    np.testing.assert_array_equal(ys, _one_point(gpr, Xs))
    Xn, yn, cnt, _ = gpr.device.ns_generation(lo, hi, Xs, ys, float(np.min(ys)), np.eye(D), 3, 1, 0, 4)
    assert Xn.shape == (0, D) and yn.shape == (0,) and cnt.shape == (0,)


def _maximize(kind, gpr, lo, hi, X0, max_iter, hooks):
    fixed, H0 = np.zeros(D, bool), np.eye(D)
    if kind == "mean":
        return gpr.device.maximize_mean(lo, hi, X0, _nan(len(X0)), fixed, H0, max_iter, 12, 1e-6, 0.0, -np.inf, hooks=hooks)
    return gpr.device.maximize_acq(lo, hi, X0, fixed, H0, float(D) ** -0.85, float(gpr.y_max), 0.0, max_iter, 12, 1e-6, 0.0,
                                   -np.inf, hooks=hooks)


@pytest.mark.parametrize("hooks", [False, True])
@pytest.mark.parametrize("kind", ["mean", "acq"])
def test_no_iterations_return_the_starts_and_traces_of_the_start_alone(kind, hooks):
    gpr, lo, hi, Lp, X0 = _model()
    out = _maximize(kind, gpr, lo, hi, X0, 0, hooks)
    np.testing.assert_array_equal(out["X"], X0)
    np.testing.assert_array_equal(out["iters"], 0)
    np.testing.assert_array_equal(out["y"], _one_point(gpr, X0))
    assert ("U_tr" in out) == hooks
    if hooks:
        assert out["U_tr"].shape == (4, 1, D) and out["G_tr"].shape == (4, 1, D)
        assert out["nhalv_tr"].shape == (4, 0) and out["reset_tr"].shape == (4, 0)
        np.testing.assert_array_equal(out["U_tr"][:, 0], (X0 - lo) / (hi - lo))
        np.testing.assert_array_equal(out["G_tr"][:, 0], out["G"])
        value = "y" if kind == "mean" else "a"
        np.testing.assert_array_equal(out[value + "_tr"][:, 0], out[value])


# ---- the hooks' regions leave the other outputs alone -------------------------------------------------------------------
def test_hmc_hooks_on_and_off_give_the_same_chains():
    gpr, lo, hi, Lp, X0 = _model()
    args = (lo, hi, X0[:2], _nan(2), Lp, 0.3, 2, 1.0, gpr.minus_inf_value, 9, 1, 3, 1)
    off = gpr.device.hmc_chains(*args, reflect=True)
    on = gpr.device.hmc_chains(*args, hooks=True, reflect=True)
    assert set(on) - set(off) == {"X_prop", "y_prop", "dH_prop", "G0"} and "nreflect" in off
    assert on["X_prop"].shape == (2, 3, D) and np.all(np.isfinite(on["G0"]))
    _assert_same(on, off, [k for k in off if k != "device_ms"])


@pytest.mark.parametrize("kind", ["mean", "acq"])
def test_maximiser_hooks_on_and_off_give_the_same_ascents(kind):
    gpr, lo, hi, Lp, X0 = _model()
    off = _maximize(kind, gpr, lo, hi, X0[:2], 3, False)
    on = _maximize(kind, gpr, lo, hi, X0[:2], 3, True)
    assert set(on) - set(off) == {"U_tr", ("y" if kind == "mean" else "a") + "_tr", "G_tr", "nhalv_tr", "reset_tr"}
    assert on["U_tr"].shape == (2, 4, D) and np.sum(on["iters"]) > 0
    _assert_same(on, off, [k for k in off if k != "device_ms"])
