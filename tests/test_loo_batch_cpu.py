"""The side-by-side ``"loo"`` fit without a GPU: the host side of ``fit_gpr_hyperparameters(objective="loo",
side_by_side=True)`` on a stand-in device whose ``loo_objective_batch`` loops over the numpy closed form
(tests/tools/loo_batch_model.py): the three ways of switching it on, the optima against the sequential fit's, the refusal
for an ``"lml"`` fit, the fall-back with its reason, copies and pickles, and the unchanged default.
"""
import copy
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loo_batch_model as lb  # noqa: E402
import loo_fit_model as lf  # noqa: E402
from oracle_device import attach  # noqa: E402

from gpry_amd import lockstep  # noqa: E402
from gpry_amd.kernels import RBF, ConstantKernel as C, WhiteKernel  # noqa: E402

BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0]])


def data(n=36, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


def make_gpr(n_restarts=3, device=None, **kw):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    kernel = C(1.0, [1e-3, 1e4]) * RBF([1.0, 1.0], [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    return attach(GaussianProcessRegressor(kernel=kernel, bounds=BOUNDS, n_restarts_optimizer=n_restarts, noise_level=1e-2,
                                           preprocessing_X=Normalize_bounds(BOUNDS), preprocessing_y=Normalize_y(),
                                           account_for_inf=None, random_state=3, **kw),
                  device if device is not None else lb.LooBatchDevice())


def fitted(how):
    """A model with the data appended and a ``"loo"`` fit switched on in one of the three ways (or sequential)."""
    X, y = data()
    gpr = make_gpr()
    if how == "attribute":
        gpr.fit_loo_side_by_side = True
        gpr.append_to_data(X, y, fit_gpr={"objective": "loo"})
    elif how == "dict":
        gpr.append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": True})
    else:
        gpr.append_to_data(X, y, fit_gpr=False)
        gpr.fit_gpr_hyperparameters(objective="loo", **({"side_by_side": True} if how == "argument" else {}))
    return gpr


@pytest.mark.parametrize("how", ["argument", "attribute", "dict"])
def test_the_three_switches_reach_the_batched_objective(how):
    gpr = fitted(how)
    dev, st = gpr.device, gpr.fit_stats
    assert st["objective"] == "loo"
    if not lockstep.available():
        print(f"no lock-step driver for this scipy ({lockstep.why()}): the fit fell back")
        assert st["side_by_side"] is False and st["why"] == lockstep.why() and dev.n_loo_batch == 0 and dev.n_loo > 3
        return
    print(f"{how}: {dev.n_loo_batch} batch calls with {dev.n_loo_rows} thetas, {dev.n_loo} single calls")
    assert st["side_by_side"] is True and st["why"] == ""
    # every round through the batch; a single call at the most, for the value at the chosen theta
    assert dev.n_loo_batch > 0 and dev.n_loo_rows >= 3 and dev.n_loo <= 1
    assert sum(st["evals_per_run"]) == dev.n_loo_rows == sum(st["evals_per_context"])
    assert st["schedule"] == "latency" and st["contexts"] == 1
    assert np.isfinite(gpr.loo_value_)
    assert gpr.log_marginal_likelihood_value_ == gpr.log_marginal_likelihood(gpr.kernel_.theta)


def test_side_by_side_optima_are_the_sequential_fit_s():
    if not lockstep.available():
        print(f"skipped: no lock-step driver for this scipy ({lockstep.why()})")
        pytest.skip(lockstep.why())
    seq, sbs = fitted("sequential"), fitted("argument")
    assert seq.fit_stats["side_by_side"] is False and sbs.fit_stats["side_by_side"] is True
    assert seq.device.n_loo_batch == 0
    assert np.array_equal(sbs.kernel_.theta, seq.kernel_.theta)
    assert sbs.loo_value_ == seq.loo_value_
    assert sbs.log_marginal_likelihood_value_ == seq.log_marginal_likelihood_value_
    # ... and the same generator state afterwards: the start points were drawn in the reference's order
    assert sbs._rng.uniform() == seq._rng.uniform()


def test_side_by_side_is_refused_for_an_lml_fit():
    X, y = data()
    gpr = make_gpr()
    gpr.append_to_data(X, y, fit_gpr=False)
    with pytest.raises(ValueError, match="side_by_side"):
        gpr.fit_gpr_hyperparameters(objective="lml", side_by_side=True)
    with pytest.raises(ValueError, match="side_by_side"):
        gpr.fit_gpr_hyperparameters(side_by_side=True)                  # the default objective is the LML
    # the attribute concerns "loo" fits alone: an LML fit of the same model is not refused and makes no batch call
    gpr.fit_loo_side_by_side = True
    gpr.fit_lockstep = False
    gpr.fit_gpr_hyperparameters(objective="lml")
    assert gpr.fit_stats["objective"] == "lml" and gpr.device.n_loo_batch == 0 and gpr.device.n_loo == 0


def test_where_the_opt_in_cannot_be_honoured_the_fit_is_sequential_and_says_why():
    X, y = data()
    # a device without the batched objective
    gpr = make_gpr(device=lf.LooDevice())
    gpr.append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": True})
    assert gpr.fit_stats["side_by_side"] is False and "loo_objective_batch" in gpr.fit_stats["why"] and gpr.device.n_loo > 3
    # a model above the batched objective's limit
    gpr = make_gpr()
    gpr.device.lml_batch_max = 16
    X2, y2 = data(140)
    gpr.n_restarts_optimizer = 2
    gpr.append_to_data(X2, y2, fit_gpr={"objective": "loo", "side_by_side": True})
    assert gpr.fit_stats["side_by_side"] is False and "lml_batch" in gpr.fit_stats["why"] and gpr.device.n_loo_batch == 0
    # lock-step switched off
    gpr = make_gpr()
    gpr.fit_lockstep = False
    gpr.append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": True})
    assert gpr.fit_stats["side_by_side"] is False and "fit_lockstep" in gpr.fit_stats["why"] and gpr.device.n_loo_batch == 0
    # one restart: nothing to step together
    gpr = make_gpr(n_restarts=1)
    gpr.append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": True})
    assert gpr.fit_stats["side_by_side"] is False and gpr.fit_stats["why"] == "one restart" and gpr.device.n_loo_batch == 0


def test_deepcopy_and_pickle_carry_the_switch():
    X, y = data()
    gpr = make_gpr(n_restarts=1)
    gpr.fit_objective = "loo"
    gpr.fit_loo_side_by_side = True
    gpr.append_to_data(X, y, fit_gpr=True)
    c = copy.deepcopy(gpr)
    assert c.fit_loo_side_by_side is True and c.fit_objective == "loo" and c.loo_value_ == gpr.loo_value_
    p = pickle.loads(pickle.dumps(gpr))
    assert p.fit_loo_side_by_side is True and p.loo_value_ == gpr.loo_value_
    assert not hasattr(copy.deepcopy(make_gpr()), "fit_loo_side_by_side")


def test_a_default_loo_fit_makes_no_batch_call_and_reports_as_before():
    gpr = fitted("sequential")
    st = gpr.fit_stats
    assert gpr.device.n_loo_batch == 0 and gpr.device.n_loo > 3
    assert st["objective"] == "loo" and st["side_by_side"] is False and "one after another" in st["why"]
    assert set(st) == {"contexts", "devices", "evals_per_context", "schedule", "side_by_side", "why", "objective"}
    assert st["contexts"] == 1 and st["schedule"] == "latency" and st["evals_per_context"] is None
    # side_by_side=False spelled out is the default
    X, y = data()
    other = make_gpr()
    other.append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": False})
    assert other.device.n_loo_batch == 0 and np.array_equal(other.kernel_.theta, gpr.kernel_.theta)
