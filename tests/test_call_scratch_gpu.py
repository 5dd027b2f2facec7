"""The call scratch of a context (csrc/common.h: CallScratch): one device buffer that the entry points with private
scratch hold one at a time, reported as ``timing("scratch_bytes")``.

* A context that has run all of them holds the largest of their footprints, not the sum, and answers each like a fresh one.
* A model of less than half the footprint gives the buffer back; the next holder allocates what it needs and no more.
* A model that only crosses a padding boundary (512 to 384 padded rows) keeps it.

Ops, inputs and the comparison of bits are those of the state-interaction harness (tests/tools/ctx_state.py).
"""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ctx_state as cs  # noqa: E402

pytestmark = pytest.mark.gpu

# the ops of the table whose entry points claim the call scratch
HOLDERS = ("lml_hessian", "predict_cov", "sample_joint", "loo", "leave_out", "predict_without", "mean_theta_grad",
           "var_theta_grad", "svm_fit", "ns_generation_phantoms", "ns_knn")
MODELS = {"a": cs.model_a(), "b": cs.model_b()}


def _device():
    from gpry_amd import _lib
    return _lib.Device(0)


def _bytes(dev):
    return dev.timing("scratch_bytes")[1]


@pytest.fixture(scope="module")
def holders():
    dev = _device()
    try:
        ops = cs.by_name(cs.table(dev)[0], HOLDERS)
    finally:
        dev.close()
    assert [o.name for o in ops] == list(HOLDERS)
    return ops


@pytest.fixture(scope="module")
def alone(holders):
    """{model: {op: (scratch_bytes after the op alone on a fresh context, its answer there)}}."""
    out = {}
    for k, case in MODELS.items():
        out[k] = {}
        for o in holders:
            dev = _device()
            try:
                cs.build(dev, case)
                assert _bytes(dev) == 0, "a context that has only been built holds no call scratch"
                answer = o(dev, case)
                out[k][o.name] = (_bytes(dev), answer)
            finally:
                dev.close()
    return out


def _run_all(dev, case, holders, want):
    done = []
    for o in holders:
        cs.compare(o(dev, case), want[o.name][1], cs.where(case, done, o.name))
        done.append(o.name)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_a_context_holds_the_largest_footprint_not_the_sum(holders, alone, model):
    case, want = MODELS[model], alone[model]
    sizes = {name: b for name, (b, _) in want.items()}
    print(f"{case.name}: scratch_bytes alone {sizes}, sum {sum(sizes.values())}")
    assert all(b > 0 for b in sizes.values()), sizes
    assert len(set(sizes.values())) >= 2, "every holder reports the same size: the comparison with the maximum says nothing"
    dev = _device()
    try:
        cs.build(dev, case)
        _run_all(dev, case, holders, want)
        assert _bytes(dev) == max(sizes.values()) < sum(sizes.values())
        _run_all(dev, case, holders[::-1], want)              # ... and once grown it stays: every holder inside a larger buffer
        assert _bytes(dev) == max(sizes.values())
    finally:
        dev.close()


def test_a_model_of_less_than_half_the_footprint_gives_the_scratch_back(holders, alone):
    a, b = MODELS["a"], MODELS["b"]
    assert 2 * cs.padded(len(b.X_)) ** 2 < cs.padded(len(a.X_)) ** 2
    dev = _device()
    try:
        cs.build(dev, a)
        _run_all(dev, a, holders, alone["a"])
        assert _bytes(dev) > 0
        cs.build(dev, b)
        assert _bytes(dev) == 0
        first = holders[-1]                                   # (a small one: the next must grow the buffer again)
        cs.compare(first(dev, b), alone["b"][first.name][1], cs.where(b, ["model a", "build b"], first.name))
        assert _bytes(dev) == alone["b"][first.name][0]
        _run_all(dev, b, holders, alone["b"])
        assert _bytes(dev) == max(s for s, _ in alone["b"].values())
    finally:
        dev.close()


def test_a_model_that_crosses_a_padding_boundary_keeps_the_scratch(holders):
    """One padding step down, at a size where the step is less than the rule's factor (2 Np^2 against the square of the
    padded size at the last growth): N = 400 to 380, 512 to 384 padded rows.  (From model a's 384 padded rows the next
    step down, 256, is already below it -- 2 * 256^2 < 384^2 -- and gives the buffer back.)"""
    big, smaller = cs.model_a(400), cs.model_a(380)
    Np, Nq = cs.padded(len(big.X_)), cs.padded(len(smaller.X_))
    assert (Np, Nq) == (512, 384) and 2 * Nq ** 2 > Np ** 2
    fresh = _device()
    try:
        cs.build(fresh, big)
        want = {o.name: (0, o(fresh, big)) for o in holders}
    finally:
        fresh.close()
    dev = _device()
    try:
        cs.build(dev, big)
        _run_all(dev, big, holders, want)
        held = _bytes(dev)
        assert held > 0
        cs.build(dev, smaller)
        assert _bytes(dev) == held
        cs.build(dev, big)
        assert _bytes(dev) == held
        _run_all(dev, big, holders, want)
        assert _bytes(dev) == held
    finally:
        dev.close()


def test_the_step_from_384_to_256_padded_rows_is_below_the_rule(holders, alone):
    """N = 300 to 250: one padding step, but 2 * 256^2 = 131072 < 147456 = 384^2, so the rule gives the buffer back."""
    a, smaller = MODELS["a"], cs.model_a(250)
    Np, Nq = cs.padded(len(a.X_)), cs.padded(len(smaller.X_))
    assert (Np, Nq) == (384, 256) and 2 * Nq ** 2 < Np ** 2
    dev = _device()
    try:
        cs.build(dev, a)
        _run_all(dev, a, holders, alone["a"])
        assert _bytes(dev) == max(s for s, _ in alone["a"].values())
        cs.build(dev, smaller)
        assert _bytes(dev) == 0
    finally:
        dev.close()
