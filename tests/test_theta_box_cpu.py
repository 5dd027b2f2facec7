"""The truth, the yardstick and the assertions of the theta-box tests (tests/tools/theta_box_model.py) without a GPU: the
long-double truth against the exact limit and against central differences of its own value, the construction of the
yardstick, the float64 V-route stand-in through every assertion of tests/test_theta_box_gpu.py (it must pass everywhere), and
the same stand-in with every kernel entry multiplied by (1 + s 2^-k), which must be rejected: the sensitivity of the
assertions in ulps of a kernel entry (profiles/theta_box.md).
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import theta_box_model as tb  # noqa: E402

LD = np.longdouble
needs_extended = pytest.mark.skipif(not tb.EXTENDED, reason="np.longdouble is no wider than float64 here")

CASES = [(N, d, kid, ti) for (N, d) in tb.SIZES for kid in range(4) for ti in range(len(tb.THETAS))]
IDS = [f"n{N}_d{d}_k{kid}_{tb.THETAS[ti][0]}" for N, d, kid, ti in CASES]
# the sensitivity: every C = 1e6 model of the two smaller sizes
SENSITIVITY = [(N, d, kid, ti) for (N, d) in tb.SIZES[:2] for kid in range(4) for ti in range(len(tb.THETAS)) if tb.THETAS[ti][1] == 1e6]
# the largest k at which the perturbed stand-in is rejected at every model of SENSITIVITY (largest_k_rejected_everywhere; run this
# file as a script to repeat the search), for all assertions and for those on the objective alone
K_REJECTED = 48
K_REJECTED_OBJECTIVE = 21


@needs_extended
@pytest.mark.parametrize("C", [1e-4, 1.0, 1e6])
def test_truth_agrees_with_the_exact_limit(C):
    X_, y_, theta = tb.grid_model(C)
    t = tb.truth(X_, y_, np.full(len(y_), tb.ALPHA), theta, 0)
    lml, gc = tb.exact_limit(y_, theta[0])
    off = t["K"] - np.diag(np.diag(t["K"]))
    assert np.max(np.abs(off)) < LD("1e-1000")            # (long double has the range for them; float64 underflows to exactly 0)
    assert abs(t["lml"] - lml) <= 1e-17 * abs(lml)
    assert abs(t["grad"][0] - gc) <= 1e-16 * max(1.0, abs(gc))
    assert np.all(np.abs(t["grad"][1:]) < LD("1e-1000"))
    # the float64 oracle reproduces the limit as well
    ol, og = tb.orc.log_marginal_likelihood(X_, y_, np.full(len(y_), tb.ALPHA), theta, 0, eval_gradient=True)
    assert abs(LD(ol) - lml) <= 1e-15 * abs(lml) and np.all(og[1:] == 0.0)


@needs_extended
@pytest.mark.parametrize("N,d,kid", [(100, 3, 3), (130, 2, 1)])
def test_truth_agrees_with_central_differences_of_its_own_value(N, d, kid):
    X_, y_ = tb.data(N, d)
    alpha = np.full(N, tb.ALPHA)
    theta = np.log(np.append(2.0, np.random.default_rng(N).uniform(0.2, 0.6, d)))
    g = tb.truth(X_, y_, alpha, theta, kid)["grad"]
    h = 1e-5
    for j in range(d + 1):
        e = np.zeros(d + 1)
        e[j] = h
        fd = (tb.truth(X_, y_, alpha, theta + e, kid)["lml"] - tb.truth(X_, y_, alpha, theta - e, kid)["lml"]) / (2 * LD(h))
        assert abs(fd - g[j]) <= 1e-7 * float(np.max(np.abs(g))), (j, fd, g[j])


@needs_extended
@pytest.mark.parametrize("case", [(100, 3, 3, tb.MODERATE), (130, 2, 0, 1), (100, 3, 1, 6)])
def test_both_routes_of_the_yardstick_lie_within_their_own_e64(case):
    m = tb.model(*case)
    tb.check_factorises_everywhere(m)
    e, t = m["e64"], m["truth"]
    assert len(e["samples"]) == 6
    for q in ("lml", "grad", "mean", "var"):
        assert all(0 <= s[q] <= e[q] for s in e["samples"]) and np.isfinite(e[q]) and e[q] > 0
    for route in (tb.oracle_route, tb.v_route):
        r = route(m["X_"], m["y_"], m["alpha"], m["theta"], m["kid"], m["Xq"])
        for q in ("lml", "grad", "mean", "var"):
            assert float(np.max(np.abs(np.asarray(r[q], dtype=LD) - t[q]))) <= e[q]


@needs_extended
def test_truth_is_what_float64_computes_where_float64_is_good():
    """A benign theta (C = 2, l in 0.2 .. 0.6, Matern-1/2: cond(K) 1e4 .. 1e5): the two float64 routes agree with the truth to
    the suite's fixed tolerances, so the truth is the same function and not merely self-consistent."""
    N, d, kid = 130, 2, 1
    X_, y_ = tb.data(N, d)
    alpha = np.full(N, tb.ALPHA)
    theta = np.log(np.append(2.0, np.random.default_rng(N).uniform(0.2, 0.6, d)))
    Xq = tb.queries(X_, theta)
    t = tb.truth(X_, y_, alpha, theta, kid, Xq)
    e = tb.yardstick(X_, y_, alpha, theta, kid, Xq, t)
    assert e["lml"] <= 1e-10 * abs(t["lml"]) and e["grad"] <= 1e-7 * np.max(np.abs(t["grad"]))
    assert e["mean"] <= 1e-8 and e["var"] <= 1e-9 * 2.0 and e["kgrad"] <= 1e-10 * np.max(np.abs(t["kgrad"]))
    assert np.isfinite(t["kgrad"]).all()


# ------------------------------------------------------------------------------------ the stand-in through the assertions
@needs_extended
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_float64_stand_in_passes_every_assertion(case):
    m = tb.model(*case)
    dev = tb.VRouteDevice()
    tb.check_objective(dev, m)
    tb.check_factor(dev, m)
    tb.check_predictions(dev, m)


@needs_extended
@pytest.mark.parametrize("C", [1e-4, 1.0, 1e6])
def test_the_float64_stand_in_passes_the_exact_limit(C):
    tb.check_exact_limit(tb.VRouteDevice(), C)


@needs_extended
@pytest.mark.parametrize("N,d", tb.SIZES)
@pytest.mark.parametrize("kid", range(4))
def test_the_float64_stand_in_passes_the_not_positive_definite_corner(N, d, kid):
    tb.check_not_positive_definite(tb.VRouteDevice(), N, d, kid)


def rejected(check, m, k):
    try:
        check(tb.VRouteDevice(k=k), m)
    except AssertionError:
        return True
    return False


def all_checks(dev, m):
    tb.check_objective(dev, m)
    tb.check_factor(dev, m)
    tb.check_predictions(dev, m)


def largest_k_rejected_everywhere(check):
    """The search behind K_REJECTED: per model the largest k at which the perturbed stand-in is rejected, and their minimum."""
    worst = {}
    for case in SENSITIVITY:
        m = tb.model(*case)
        k = 52
        while k > 0 and not rejected(check, m, k):
            k -= 1
        worst[m["name"]] = k
    return min(worst.values()), worst


@needs_extended
@pytest.mark.parametrize("check,k", [(all_checks, K_REJECTED), (tb.check_objective, K_REJECTED_OBJECTIVE)], ids=["all", "objective"])
def test_a_perturbed_stand_in_is_rejected(check, k):
    """Every kernel entry times (1 + s 2^-k): rejected at every C = 1e6 model at k, that is at 2^(52 - k) ulps of an entry."""
    for case in SENSITIVITY:
        assert rejected(check, tb.model(*case), k), (case, k)


if __name__ == "__main__":
    for check in (all_checks, tb.check_objective):
        print(check.__name__, *largest_k_rejected_everywhere(check))
