"""One context, many callers: no entry point may change the answer of any other, and a context that has held other
models answers like a fresh one (harness: tests/tools/ctx_state.py; the harness itself: tests/test_ctx_state_cpu.py).

* Every op of the table is bit-repeatable on a fresh context.
* Every ordered pair (A immediately before B) of ops, on three models, against each op's answer on a context that has only
  been built: n orderings of the n ops per model.
* Every op between the objective evaluation that arms the adoption cache and the factorisation that adopts.
* One context through a chain of eleven models, probed after every transition against a fresh context; sessions and
  pools that must not survive a transition; a failed append; capacities that grow only when a larger model arrives.
* The fresh context against the oracle, so that "equal to a fresh context" cannot mean "equally wrong".
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ctx_state as cs  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = {"a": cs.model_a(), "b": cs.model_b(), "c": cs.model_c()}
N_OPS = len(cs.OPS) + len(cs.OPS) % 2
ORDERS = list(cs.sequences(N_OPS))

# Ops whose answer may differ from run to run because the code says so (a state-dependent choice of path, an unordered
# sum): {name: (the code's own comment, rtol of the op's own test file against the oracle)}.  Expected to stay empty.
NOT_BIT_REPEATABLE = {}
TOLERANT = {k: v[1] for k, v in NOT_BIT_REPEATABLE.items()}


def _device():
    from gpry_amd import _lib
    return _lib.Device(0)


@pytest.fixture(scope="module")
def ops():
    dev = _device()
    try:
        return cs.table(dev)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def fresh(ops):
    """{model: (each op's answer on a context that has run build and nothing else, its answer to the same call again)}."""
    out = {}
    for k, case in MODELS.items():
        again = {}
        out[k] = (cs.baselines(_device, case, ops[0], again), again)
    return out


def test_no_op_is_skipped(ops):
    table, skipped = ops
    assert skipped == [] and len(table) == N_OPS
    assert all(o.model_neutral for o in table)


def test_the_list_of_ops_that_are_not_bit_repeatable_cannot_grow_silently():
    assert len(NOT_BIT_REPEATABLE) <= 3
    assert set(NOT_BIT_REPEATABLE) <= {o.name for o in cs.OPS}
    assert all(reason.strip() and 0.0 < rtol <= 1e-6 for reason, rtol in NOT_BIT_REPEATABLE.values())


@pytest.mark.parametrize("model", sorted(MODELS))
def test_every_op_is_bit_repeatable_on_a_fresh_context(ops, fresh, model):
    first, again = fresh[model]
    case = MODELS[model]
    lml, grad, info = first["lml_nonpd"]
    assert lml == -np.inf and not grad.any() and info > 0, "lml_nonpd is meant to meet a matrix that is not positive definite"
    value, grad, info = first["loo_objective_nonpd"]
    assert value == -np.inf and not grad.any() and info > 0, "loo_objective_nonpd is meant to meet a matrix that is not positive definite"
    for o in ops[0]:
        if o.name in NOT_BIT_REPEATABLE:
            assert cs.close_enough(again[o.name], first[o.name], TOLERANT[o.name]), o.name
        else:
            cs.compare(again[o.name], first[o.name], cs.where(case, [o.name], o.name))


@pytest.mark.parametrize("i", range(N_OPS))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_every_ordered_pair_of_ops(ops, fresh, model, i):
    case = MODELS[model]
    dev = _device()
    try:
        cs.build(dev, case)
        cs.run_sequence(dev, case, [ops[0][k] for k in ORDERS[i]], fresh[model][0], tolerant=TOLERANT)
    finally:
        dev.close()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_every_op_between_arming_and_adoption(ops, fresh, model):
    """lml at the model's own theta arms the adoption of its factor by the next factorize; an op in between that borrows
    the scratch matrices has to disarm it (gpry_kernel_train does: "dW is about to be overwritten").  Whatever runs in
    between, the factorisation gives the factor of a fresh context."""
    case = MODELS[model]
    table = {o.name: o for o in ops[0]}
    dev = _device()
    try:
        cs.build(dev, case)
        for o in ops[0]:
            if o.name in ("refactorize", "lml_own"):
                continue
            table["lml_own"](dev, case)
            o(dev, case)
            cs.compare(table["refactorize"](dev, case), fresh[model][0]["refactorize"],
                       cs.where(case, ["...", "lml_own", o.name], "refactorize"))
    finally:
        dev.close()


def _capacity(dev):
    return dev.timing("capacity_rows")[1], dev.timing("capacity_cols")[1]


def test_model_transitions_on_one_context(ops):
    """One context through the chain of ``ctx_state.chain`` without ever being closed.  After every transition: the
    Kriging-believer session registered before it is gone (or, where no call touched the factor, answers like a fresh
    one); the resident pool is swept under the new model or, after a change of width, refused; and every probe gives the
    bits of a fresh context taken through ``build`` for that model alone."""
    from gpry_amd._lib import GpryHipError
    probes = cs.by_name(ops[0], cs.PROBES)
    assert [o.name for o in probes] == list(cs.PROBES)
    steps = cs.chain()
    sizes = [len(s.case.X_) + sum(len(a[0]) for a in s.case.appends) for s in steps]
    assert sizes == [300, 300, 303, 393, 100, 129, 128, 1, 1100, 1100, 300]
    assert cs.padded(sizes[2]) == cs.padded(sizes[1]) < cs.padded(sizes[3])       # append 3: inside; append 90: past
    n_kb = sum(cs.KB_ROWS)
    dev, history, caps, prev = _device(), [], [], None
    try:
        for step in steps:
            case = step.case
            step.apply(dev)
            history.append(step.label)
            caps.append(_capacity(dev))
            other = _device()
            try:
                cs.build(other, case)
                want = cs.probe(other, case, probes)
            finally:
                other.close()
            if prev is not None:
                at = f"{case.name} after {' => '.join(history)}"
                # the session registered before the transition: gone with the factor it was started on
                if step.keeps_factor:
                    cs.compare(cs.flat(dev.kb_gram(n_kb - 1, n_kb)), want["kb_session"][4:6], at + ": kb_gram of the standing session")
                else:
                    with pytest.raises(GpryHipError):
                        dev.kb_gram(0, n_kb)
                # the resident pool: X == NULL re-uses it under the new model (include/gpry_hip.h), rows of another
                # width are no pool of this model
                with cs.option(dev, sweep_chunk=1024):
                    if step.same_width:
                        out = dev.sweep_logexp(None, case.zeta, case.baseline, case.sigma_n, M=cs.SWEEP_M)
                        cs.compare(cs.flat((out, cs._topk(dev))), want["sweep"][:len(cs.flat(out)) + 5], at + ": sweep of the resident pool")
                    else:
                        with pytest.raises(GpryHipError):
                            dev.sweep_logexp(None, case.zeta, case.baseline, case.sigma_n, M=cs.SWEEP_M)
            cs.compare_probes(cs.probe(dev, case, probes), want, case, history)
            refused = {k for k, v in want.items() if v and isinstance(v[0], str)}
            assert refused == ({"hessian_mean"} if case.kid == cs.M12 else set()), (case.name, refused)    # (no Matern-1/2 Hessian)
            prev = step
        # the buffers hold the padded size in use at every step, and grow only when a larger model arrives
        rows = [c[0] for c in caps]
        assert all(r >= cs.padded(n) for r, n in zip(rows, sizes)) and rows == sorted(rows)
        assert rows[2] == rows[1] and rows[3] > rows[2]
        assert caps[10] == caps[8], caps
    finally:
        dev.close()


def test_a_resident_pool_of_another_width_is_refused():
    """Regression (found by test_model_transitions_on_one_context, transition 4 => 5): after gpry_set_train with another
    d, gpry_sweep_logexp with X == NULL and the old pool's size read the resident rows with the new stride and answered.
    The pool goes with the width it was uploaded in; a model of the same width keeps it."""
    from gpry_amd._lib import GpryHipError
    narrow, wide, narrow2 = cs.Case("d=5", 60, 5, cs.M52, seed=21), cs.model_b(), cs.Case("d=5 again", 70, 5, cs.M32, seed=22)
    pool = cs.sweep_pool(narrow)
    dev = _device()
    try:
        cs.build(dev, narrow)
        dev.sweep_logexp(pool, narrow.zeta, narrow.baseline, narrow.sigma_n)
        cs.build(dev, narrow2)                                  # same width: the pool stands, under the new model
        again = dev.sweep_logexp(None, narrow2.zeta, narrow2.baseline, narrow2.sigma_n, M=cs.SWEEP_M)
        direct = dev.sweep_logexp(pool, narrow2.zeta, narrow2.baseline, narrow2.sigma_n)
        cs.compare(cs.flat(again), cs.flat(direct), "sweep of the resident pool under a model of the same width")
        cs.build(dev, wide)
        for case in (wide, narrow):
            if case is narrow:
                cs.build(dev, narrow)                           # back to the old width: the pool is still gone
            with pytest.raises(GpryHipError, match="no resident candidate set"):
                dev.sweep_logexp(None, case.zeta, case.baseline, case.sigma_n, M=cs.SWEEP_M)
            with pytest.raises(GpryHipError):
                dev.sweep_topk(10)
        assert np.all(np.isfinite(dev.predict(narrow.points("after", 5))))
    finally:
        dev.close()


def test_the_resident_predict_kernel_waits_for_the_restored_coordinates():
    """Regression (found by test_every_ordered_pair_of_ops[b-12], lml_nonpd -> predict_1_served, in one run of the whole
    suite out of five of this file): the first served predict after an objective evaluation puts the prediction factor's
    scaled coordinates back with a launch on the context's stream and starts the resident kernel on a stream of its own,
    which read the buffer while 3 of the 9 workgroups of that launch had not written yet (-48.86 for -10.78, the value
    that exactly those stale rows give).  gpry_predict now waits for the restoring launch before it starts the kernel.
    The window opens only when the device delays that launch: on an idle GPU this test passed before the fix as well.  It
    pins the pair where the window is widest -- a restoring launch of 320 workgroups, and an evaluation whose scaled
    coordinates are all but zero, so that a single stale row shows."""
    case = cs.Case("N=4000, d=20, RBF", 4000, 20, cs.RBF, seed=31, xmap=False, scale=1.0)
    x = case.points("served", 1)
    dev = _device()
    try:
        cs.build(dev, case)
        want = dev.predict(x)
        launches = dev.serve_stats()[0]
        assert launches == 1                                      # (the resident kernel did answer)
        for i in range(16):
            lml, info = dev.lml(case.theta_nonpd(), False)        # stops the kernel, leaves its own scaled coordinates
            assert info > 0 and lml == -np.inf
            got = dev.predict(x)
            assert got[0] == want[0], f"served predict {i} after an objective evaluation: {got[0]!r} != {want[0]!r}"
        assert dev.serve_stats()[0] == launches + 16
    finally:
        dev.close()


def test_a_failed_append_leaves_no_prediction(ops):
    dev, case = _device(), cs.failed_append_case()
    try:
        cs.build(dev, case)
        assert dev.append_rows(*cs.bad_border(case)) == len(case.X_) + 1            # 1-based column of the failing pivot
        got = cs.probe(dev, case, cs.by_name(ops[0], cs.PREDICTION_PROBES))
        assert len(got) == len(cs.PREDICTION_PROBES)
        assert all(v and v[0] == "raised" for v in got.values()), {k: v[:2] for k, v in got.items()}
        # ... and a new factorisation puts everything back
        cs.build(dev, case)
        other = _device()
        try:
            cs.build(other, case)
            probes = cs.by_name(ops[0], cs.PROBES)
            cs.compare_probes(cs.probe(dev, case, probes), cs.probe(other, case, probes), case, ["failed append", "build"])
        finally:
            other.close()
    finally:
        dev.close()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_the_fresh_context_agrees_with_the_oracle(model):
    """Tolerances: the top of tests/test_hip_parity.py (mean 1e-8, variance 1e-9 C, LML 1e-10, gradient 1e-7 of its
    largest entry) and, for the acquisition, that file's sweep test (1e-6)."""
    case = MODELS[model]
    dev, ref = _device(), OracleDevice()
    try:
        cs.build(dev, case)
        cs.build(ref, case)
        X = case.points("anchor", 200, margin=0.03)
        (mean, std), (rm, rs) = dev.predict(X, return_std=True), ref.predict(X, return_std=True)
        C = np.exp(case.theta[0]) * case.y_std ** 2
        print(f"{case.name}: mean {np.max(np.abs(mean - rm)) / max(1.0, np.max(np.abs(rm))):.2e}, "
              f"var {np.max(np.abs(std ** 2 - rs ** 2)) / C:.2e}")
        assert np.max(np.abs(mean - rm)) <= 1e-8 * max(1.0, np.max(np.abs(rm)))
        assert np.max(np.abs(std ** 2 - rs ** 2)) <= 1e-9 * C
        (lml, grad, info), (rl, rg, _) = dev.lml(case.theta_other(1), True), ref.lml(case.theta_other(1), True)
        print(f"lml {abs(lml - rl) / abs(rl):.2e}, grad {np.max(np.abs(grad - rg)) / np.max(np.abs(rg)):.2e}")
        assert info == 0 and abs(lml - rl) <= 1e-10 * abs(rl)
        assert np.max(np.abs(grad - rg)) <= 1e-7 * np.max(np.abs(rg))
        pool = cs.sweep_pool(case)
        out = dev.sweep_logexp(pool, case.zeta, case.baseline, case.sigma_n)
        want = ref.sweep_logexp(pool, case.zeta, case.baseline, case.sigma_n)
        assert out["n_nan"] == 0 and np.array_equal(np.isneginf(out["acq"]), np.isneginf(want["acq"]))
        ok = np.isfinite(want["acq"])
        assert ok.sum() > cs.SWEEP_M // 2
        print(f"acq {np.max(np.abs(out['acq'][ok] - want['acq'][ok])):.2e} over {ok.sum()} candidates")
        np.testing.assert_allclose(out["acq"][ok], want["acq"][ok], rtol=1e-6, atol=1e-6)
    finally:
        dev.close()
