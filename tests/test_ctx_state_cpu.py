"""The state-interaction harness (tests/tools/ctx_state.py) checked on its own, without a GPU.

* ``sequences(n)`` holds every ordered pair of ops exactly once -- asserted, not taken on trust.
* The whole harness against ``OracleDevice``: the test double keeps no state between calls beyond the model, so the
  every-pair and the transition runs must pass there with exact equality.  A failure here is an order dependence of the
  harness itself (a shared generator, an input array that an op changed).
* A deliberately stateful stub, whose ``lml`` makes the next ``predict`` wrong by one ulp, must make the harness fail
  and name the pair: the harness's own mutation test.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ctx_state as cs  # noqa: E402

N_REAL = len(cs.OPS) + len(cs.OPS) % 2          # the table against the library: nothing skipped, padded to even

# small models: what is under test here is the harness, and the double's arithmetic costs the same at every size
CASES = {"a": cs.model_a(40), "b": cs.model_b(30)}


@pytest.mark.parametrize("n", sorted({2, 4, 26, 50, 54, N_REAL}))      # (50, 54: the table before later ops joined it)
def test_sequences_hold_every_ordered_pair_exactly_once(n):
    seqs = list(cs.sequences(n))
    assert len(seqs) == n
    pairs = {}
    for s in seqs:
        assert sorted(s) == list(range(n))                  # an ordering of all n ops
        for a, b in zip(s[:-1], s[1:]):
            pairs[(a, b)] = pairs.get((a, b), 0) + 1
    assert len(pairs) == n * (n - 1) and set(pairs.values()) == {1}
    assert all(a != b for a, b in pairs)


def test_sequences_refuse_an_odd_table():
    with pytest.raises(ValueError):
        list(cs.sequences(7))
    assert N_REAL % 2 == 0 and len(cs.table(OracleDevice())[0]) % 2 == 0


def test_the_table_starts_one_path_with_a_borrower_between_arming_and_adoption():
    names = [o.name for o in cs.OPS] + ["sync"] * (len(cs.OPS) % 2)
    assert any([names[i] for i in s[:3]] == ["lml_own", "kernel_train", "refactorize"] for s in cs.sequences(N_REAL))


def test_op_inputs_depend_on_the_case_alone():
    """Two draws of an op's inputs are equal and do not share memory; cases of one width share them."""
    a, b = cs.model_a(40), cs.model_a(50)
    p, q = a.points("x", 7), a.points("x", 7)
    assert np.array_equal(p, q) and not np.shares_memory(p, q)
    assert np.array_equal(p, b.points("x", 7)) and not np.array_equal(p, a.points("y", 7))


@pytest.fixture(scope="module")
def oracle_runs():
    """(ops the double can run, names it cannot, baselines per model)."""
    ops, skipped = cs.table(OracleDevice())
    return ops, skipped, {k: cs.baselines(OracleDevice, c, ops) for k, c in CASES.items()}


def test_the_run_against_the_double_is_not_vacuous(oracle_runs):
    ops, skipped, base = oracle_runs
    assert len(ops) >= 8 and len(ops) % 2 == 0, (len(ops), skipped)
    assert {"lml_other", "lml_nonpd", "predict_5_std", "predict_3000_std", "sweep", "refused_predict_columns"} <= {o.name for o in ops}
    for k, c in CASES.items():
        lml, grad, info = base[k]["lml_nonpd"]
        assert lml == -np.inf and not grad.any() and info > 0            # a verdict
        assert all(len(base[k][o.name]) > 0 for o in ops if o.name not in ("sync", "microbench"))


@pytest.mark.parametrize("model", sorted(CASES))
def test_every_ordered_pair_on_the_stateless_double(oracle_runs, model):
    ops, _, base = oracle_runs
    case = CASES[model]
    for seq in cs.sequences(len(ops)):
        dev = OracleDevice()
        cs.build(dev, case)
        cs.run_sequence(dev, case, [ops[i] for i in seq], base[model])


def small_chain():
    return cs.chain(sizes=(40, 30, 33, 32, 1, 60), k_inside=3, k_past=20)


def test_model_transitions_on_the_stateless_double(oracle_runs):
    ops, _, _ = oracle_runs
    probes = cs.by_name(ops, cs.PROBES)
    assert len(probes) >= 6
    dev, history = OracleDevice(), []
    for step in small_chain():
        step.apply(dev)
        history.append(step.label)
        got = cs.probe(dev, step.case, probes)
        fresh = OracleDevice()
        cs.build(fresh, step.case)
        cs.compare_probes(got, cs.probe(fresh, step.case, probes), step.case, history)


def test_a_failed_append_leaves_no_prediction_on_the_double(oracle_runs):
    ops, _, _ = oracle_runs
    dev, case = OracleDevice(), cs.failed_append_case()
    cs.build(dev, case)
    assert dev.append_rows(*cs.bad_border(case)) > 0
    got = cs.probe(dev, case, cs.by_name(ops, cs.PREDICTION_PROBES))
    assert got and all(v and v[0] == "raised" for v in got.values()), got


class LeakyDevice(OracleDevice):
    """``lml`` leaves a flag behind that makes the next ``predict`` wrong by one ulp."""

    dirty = False

    def lml(self, theta, eval_gradient=False):
        self.dirty = True
        return super().lml(theta, eval_gradient)

    def predict(self, X, return_std=False, mask=None):
        out = super().predict(X, return_std=return_std, mask=mask)
        if self.dirty:
            self.dirty = False
            mean = out[0] if return_std else out
            mean[...] = np.nextafter(mean, np.inf)
        return out


def test_a_stateful_device_is_caught_and_the_pair_is_named(oracle_runs):
    ops, _, base = oracle_runs
    case = CASES["a"]
    failures = []
    for seq in cs.sequences(len(ops)):
        dev = LeakyDevice()
        cs.build(dev, case)
        cs.run_sequence(dev, case, [ops[i] for i in seq], base["a"], collect=failures)
    hit = [msg for prev, name, msg in failures if (prev, name) == ("lml_other", "predict_5_std")]
    assert len(hit) == 1 and "lml_other -> predict_5_std" in hit[0] and case.name in hit[0], failures[:3]
    # every op that reads predict straight after an op that evaluates the objective is reported
    lml_ops = {o.name for o in ops if o.name.startswith("lml_") or o.name == "opt_gemm_dma"}
    readers = {"predict_1_served", "predict_1_launched", "predict_5_std", "predict_17_std", "predict_130_std",
               "predict_3000_std", "predict_masked", "sweep", "sweep_pruned", "opt_predict_small", "opt_sweep_upload",
               "opt_cross_mfma"}
    assert readers <= {o.name for o in ops}
    named = {(prev, name) for prev, name, _ in failures}
    assert {(a, b) for a in lml_ops for b in readers} <= named
    # ... and the plain double gives none (the same runs as test_every_ordered_pair_on_the_stateless_double, collected)
    clean = []
    dev = OracleDevice()
    cs.build(dev, case)
    cs.run_sequence(dev, case, ops, base["a"], collect=clean)
    assert clean == []
