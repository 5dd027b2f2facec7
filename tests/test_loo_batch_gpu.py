"""``gpry_loo_objective_batch`` on the device: B thetas of the leave-one-out fit objective through one chain of launches,
and the side-by-side ``"loo"`` fit on top of it.  The invariant under test is the project's own: per theta, value, gradient
and info of a batched call are bit for bit those of ``gpry_loo_objective`` on the same model -- whatever B, the position in
the batch, the chunking and the neighbours (a not-positive-definite one included).

Models: tests/tools/loo_fit_model.py (``problem``, the closed forms); affine settings as in test_loo_fit_gpu.py.  Shapes, the
smallest at which each piece can go wrong: (50, 1) 128 padded rows, the routing edge, one partly filled tile; (130, 2) first
size past 128; (333, 5) 384 padded rows; (300, 17) traces width class 24; (1100, 8) split / stream-K products and the split
of the Gram product.  All four kernels at the two small shapes, one each at the others, with and without the white term.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loo_fit_model as lf  # noqa: E402

pytestmark = pytest.mark.gpu

W = 0x10
Y_MEAN, Y_STD = 0.3, 1.7

CASES = [(N, d, kid, white) for (N, d) in [(50, 1), (130, 2)] for kid in range(4) for white in (False, True)]
CASES += [(333, 5, 3, False), (333, 5, 1, True), (300, 17, 0, False), (300, 17, 2, True), (1100, 8, 0, False), (1100, 8, 3, True)]
IDS = [f"n{N}_d{d}_k{kid}{'_w' if white else ''}" for N, d, kid, white in CASES]


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


def load(dev, N, d, kid, white):
    X_, y_, a, theta = lf.problem(N, d, seed=N + d, white=white)
    dev.set_train(X_, y_, a)
    dev.set_theta(kid | W if white else kid, theta)
    dev.set_affine(None, None, Y_MEAN, Y_STD)
    return X_, y_, a, theta


def thetas_of(theta, B=5):
    """The model's theta and fixed perturbations of it (row 0: theta itself), well inside the bounds of a fit."""
    steps = np.array([0.0, 0.1, -0.15, 0.05, -0.07, 0.12, -0.03])
    T = np.repeat(np.asarray(theta, dtype=float)[None, :], B, axis=0)
    for j in range(B):
        T[j] += steps[j % len(steps)] * np.where(np.arange(len(theta)) % 2 == 0, 1.0, -0.6) + 0.01 * (j // len(steps))
    return T


def singles(dev, T):
    return [dev.loo_objective(T[j], True) for j in range(len(T))]


def rows_equal(batch, single_list, rows=None):
    val, grad, info = batch
    rows = range(len(single_list)) if rows is None else rows
    for j, s in zip(rows, single_list):
        assert val[j] == s[0] or (np.isneginf(val[j]) and np.isneginf(s[0])), (j, val[j], s[0])
        assert np.array_equal(grad[j], s[1]), j
        assert info[j] == s[2], j


_cache = {}


def evaluated(dev, case):
    """Everything the tests of one model need, computed once: batched and single answers and the two numpy formulations."""
    if case in _cache:
        return _cache[case]
    N, d, kid, white = case
    X_, y_, a, theta = load(dev, *case)
    T = thetas_of(theta)
    r = dict(theta=theta, T=T)
    r["single"] = singles(dev, T)
    r["batch"] = {B: dev.loo_objective_batch(T[:B], True) for B in (1, 2, 5)}
    r["value_only"] = dev.loo_objective_batch(T, False)
    # theta 0 at row 4 of another batch: other neighbours, another position
    T2 = thetas_of(theta + 0.02)
    T2[4] = T[0]
    r["moved"] = dev.loo_objective_batch(T2, True)
    r["a"] = lf.loo_explicit(X_, y_, a, theta, kid, white)
    r["b"] = lf.loo_one_product(X_, y_, a, theta, kid, white)
    _cache[case] = r
    return r


# ------------------------------------------------------------------------------------ 1. bits against the single call
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_of_a_batch_have_the_bits_of_single_calls(dev, case):
    N, d, kid, white = case
    r = evaluated(dev, case)
    for B in (1, 2, 5):
        val, grad, info = r["batch"][B]
        assert val.shape == (B,) and grad.shape == (B, d + 1 + int(white)) and info.shape == (B,)
        assert not info.any() and np.isfinite(val).all()
        rows_equal(r["batch"][B], r["single"][:B])
    v, info = r["value_only"]
    assert np.array_equal(v, r["batch"][5][0]) and not info.any()


# ------------------------------------------------------------------------------------ 2. neighbours, position, chunking
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_bits_at_another_position_among_other_neighbours(dev, case):
    r = evaluated(dev, case)
    val, grad, info = r["moved"]
    assert val[4] == r["batch"][5][0][0] and np.array_equal(grad[4], r["batch"][5][1][0]) and info[4] == 0
    assert val[0] != r["batch"][5][0][0]                       # (the other batch really is another one)


def two_sets_mb(dev):
    """``lml_batch_mb`` at which exactly two scratch sets of the last batched call's layout fit: the arena holds
    floor(mb * 2^20 / (8 * set)) sets, the set's size reported by the context ("batch_set_doubles")."""
    per_set = 8 * dev.timing("batch_set_doubles")[1]
    assert per_set > 0
    mb = -(-2 * per_set // (1 << 20))
    assert (mb << 20) // per_set == 2, (mb, per_set)
    return mb


@pytest.mark.parametrize("case", [(50, 1, 0, False), (130, 2, 3, True), (1100, 8, 3, True)])
def test_chunks_of_two_and_scratch_sets_of_nans_change_nothing(dev, case):
    r = evaluated(dev, case)
    load(dev, *case)
    ref = dev.loo_objective_batch(r["T"], True)
    rows_equal(ref, r["single"])
    assert dev.timing("batch_chunk")[1] == 5
    mb0, dbg0 = dev.get_option("lml_batch_mb"), dev.get_option("panel_debug")
    try:
        dev.set_option("lml_batch_mb", two_sets_mb(dev))
        out = dev.loo_objective_batch(r["T"], True)             # chunks of 2, 2, 1
        assert dev.timing("batch_chunk")[1] == 2
        for x, y in zip(ref, out):
            assert np.array_equal(x, y)
        dev.set_option("panel_debug", dbg0 | 128)               # every scratch set starts as NaNs
        out = dev.loo_objective_batch(r["T"], True)
        for x, y in zip(ref, out):
            assert np.array_equal(x, y)
        dev.set_option("lml_batch_mb", mb0)
        out = dev.loo_objective_batch(r["T"], True)
        assert dev.timing("batch_chunk")[1] == 5
        for x, y in zip(ref, out):
            assert np.array_equal(x, y)
    finally:
        dev.set_option("lml_batch_mb", mb0)
        dev.set_option("panel_debug", dbg0)


def test_ninety_seven_thetas_cross_the_chunk_limit(dev):
    case = (130, 2, 2, True)
    r = evaluated(dev, case)
    load(dev, *case)
    T = thetas_of(r["theta"], 97)
    T[96] = r["T"][3]
    val, grad, info = dev.loo_objective_batch(T, True)
    assert dev.timing("batch_chunk")[1] == 96 and not info.any()
    rows_equal((val, grad, info), r["single"], rows=range(5))               # rows 0 .. 4 are the model's five
    assert val[96] == r["single"][3][0] and np.array_equal(grad[96], r["single"][3][1])      # the chunk of one
    for j in (40, 95):
        rows_equal((val, grad, info), [dev.loo_objective(T[j], True)], rows=[j])


# ------------------------------------------------------------------------------------ 3. a non-PD theta in the middle
@pytest.mark.parametrize("N,d,kid", [(64, 2, 0), (200, 3, 3)])
def test_not_positive_definite_in_the_middle_and_the_calls_after_it(dev, N, d, kid):
    """Every row twice, no noise (test_loo_fit_gpu.py's construction), a white term: positive definite where w is 1e-3, not
    where w underflows against C."""
    X_, y_, a, theta = lf.problem(N, d, seed=N + d, white=True)
    Xd = X_.copy()
    Xd[N // 2:] = Xd[:N - N // 2]
    dev.set_train(Xd, y_, np.zeros(N))
    dev.set_theta(kid | W, theta)
    dev.set_affine(None, None, Y_MEAN, Y_STD)
    T = thetas_of(theta)
    T[:, -1] = np.log(1e-3)
    T[2] = theta                                    # (the matrix of test_loo_fit_gpu.py's case, bit for bit: C + w rounds to C)
    T[2, -1] = -100.0
    one = singles(dev, T)
    assert one[2][0] == -np.inf and one[2][2] > 0 and not one[2][1].any()        # the construction does what it is for
    assert all(s[2] == 0 and np.isfinite(s[0]) for j, s in enumerate(one) if j != 2)
    val, grad, info = dev.loo_objective_batch(T, True)
    assert val[2] == -np.inf and not grad[2].any() and info[2] > 0
    rows_equal((val, grad, info), one)
    v, i2 = dev.loo_objective_batch(T, False)
    assert np.array_equal(v, val) and np.array_equal(i2, info)
    # the next batched call and the next single call answer normally
    keep = [0, 1, 3, 4]
    rows_equal(dev.loo_objective_batch(T[keep], True), [one[j] for j in keep])
    s = dev.loo_objective(T[1], True)
    assert s[0] == one[1][0] and np.array_equal(s[1], one[1][1]) and s[2] == 0


def test_refused_arguments_leave_the_context_answering(dev):
    case = (130, 2, 1, True)
    r = evaluated(dev, case)
    load(dev, *case)
    bad = r["T"].copy()
    bad[3, 1] = np.nan
    with pytest.raises(Exception, match="finite"):
        dev.loo_objective_batch(bad, True)
    with pytest.raises(Exception):
        dev.loo_objective_batch(np.empty((0, r["T"].shape[1])), True)
    with pytest.raises(ValueError):
        dev.loo_objective_batch(r["T"][:, :-1], True)
    rows_equal(dev.loo_objective_batch(r["T"], True), r["single"])


# ------------------------------------------------------------------------------------ 4. against the closed form
def bounds(r, N):
    """(value, gradient) deviations allowed, test_loo_fit_gpu.py's: ten times (a) against (b), not below the LML's bounds."""
    (va, ga), (vb, gb) = r["a"], r["b"]
    big = np.max(np.abs(gb))
    return max(10 * abs(va - vb), 1e-10 * (abs(vb) + N)), max(10 * np.max(np.abs(ga - gb)), 1e-7 * big)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batched_value_and_gradient_against_the_closed_form(dev, case):
    N, d, kid, white = case
    r = evaluated(dev, case)
    val, grad, info = r["batch"][5]
    vb, gb = r["b"]
    tol_v, tol_g = bounds(r, N)
    print(f"loo_batch {IDS[CASES.index(case)]}: value dev {abs(val[0] - vb):.2e} (allowed {tol_v:.2e}), "
          f"grad dev {np.max(np.abs(grad[0] - gb)):.2e} (allowed {tol_g:.2e})")
    assert info[0] == 0
    assert abs(val[0] - vb) <= tol_v
    assert np.max(np.abs(grad[0] - gb)) <= tol_g


# ------------------------------------------------------------------------------------ 5. the white term per theta
@pytest.mark.parametrize("case", [(50, 1, 2, True), (130, 2, 0, True), (1100, 8, 3, True)])
def test_white_entry_is_scaled_by_the_rows_own_w(dev, case):
    r = evaluated(dev, case)
    load(dev, *case)
    T = np.repeat(r["theta"][None, :], 2, axis=0)
    T[1, -1] += 1.0                                         # the same model but for w: e times the context's
    one = singles(dev, T)
    val, grad, info = dev.loo_objective_batch(T, True)
    assert grad[0, -1] == one[0][1][-1] and grad[1, -1] == one[1][1][-1]
    assert grad[0, -1] != grad[1, -1]
    rows_equal((val, grad, info), one)
    # ... and the other way round: the context's w is row 1's
    rows_equal(dev.loo_objective_batch(T[::-1], True), one[::-1])


# ------------------------------------------------------------------------------------ 6. state
def snapshot(dev, theta_other, Xq):
    """The answers of the other entry points, in a fixed order."""
    out = [dev.lml(theta_other, True)]
    assert dev.factorize() == 0
    out.append(dev.get_factor())
    out.append(dev.predict(Xq, return_std=True))
    loo = dev.loo()
    out.append([loo[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")])
    out.append(dev.loo_objective(theta_other, True))
    sw = dev.sweep_logexp(Xq, 1.0, 0.5, 0.01)
    out.append(sw[0] if isinstance(sw, tuple) else sw)
    return out


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("case", [(50, 1, 1, True), (200, 3, 3, True), (1100, 8, 3, False)])
def test_every_other_entry_point_answers_as_if_the_batch_had_not_been_made(dev, case):
    N, d, kid, white = case
    X_, y_, a, theta = load(dev, *case)
    Xq = np.random.default_rng(2).uniform(0, 1, (300, d))
    other = theta.copy()
    other[:d + 1] += 0.1
    T = thetas_of(theta - 0.15)
    before = snapshot(dev, other, Xq)
    mean_before = dev.predict(Xq[:3])
    lml_before = dev.lml_batch(T, True)
    val, grad, info = dev.loo_objective_batch(T, True)
    assert not info.any() and np.isfinite(val).all()
    assert np.array_equal(dev.predict(Xq[:3]), mean_before)            # the factor held for prediction, straight away
    assert same_bits(dev.lml_batch(T, True), lml_before)               # the arena is shared, the layouts differ
    assert same_bits(dev.loo_objective_batch(T, True), (val, grad, info))
    after = snapshot(dev, other, Xq)
    for k, (x, y) in enumerate(zip(before, after)):
        assert same_bits(x, y), k
    # the factor cache of gpry_lml: an evaluation at the model's theta, then the batch, then a factorisation
    dev.lml(theta, True)
    dev.loo_objective_batch(T, True)
    assert dev.factorize() == 0
    assert same_bits(dev.get_factor(), before[1])
    # the context's theta is still the model's
    assert same_bits(dev.predict(Xq, return_std=True), before[2])


def test_stage_timer_of_a_chunk(dev):
    case = (130, 2, 0, False)
    r = evaluated(dev, case)
    load(dev, *case)
    dev.timing_reset()
    dev.loo_objective_batch(r["T"], True)
    ms, count = dev.timing("loo_batch")
    assert count == 1 and ms > 0.0
    assert dev.timing("loo_gram")[1] == 1 and dev.timing("loo_traces")[1] == 1      # one chain for the five thetas


# ------------------------------------------------------------------------------------ 7. the fall-back routes
@pytest.mark.parametrize("case", [(130, 2, 3, True), (333, 5, 3, False)])
def test_above_the_batch_limit_the_thetas_go_one_after_another(dev, case):
    r = evaluated(dev, case)
    load(dev, *case)
    lim0, mb0 = dev.get_option("lml_batch"), dev.get_option("lml_batch_mb")
    try:
        dev.set_option("lml_batch", 128)                    # below the model's padded size
        dev.timing_reset()
        out = dev.loo_objective_batch(r["T"], True)
        assert dev.timing("loo_batch")[1] == 0 and dev.timing("loo_traces")[1] == 5
        rows_equal(out, r["single"])
        assert np.array_equal(dev.loo_objective_batch(r["T"], False)[0], out[0])
        dev.set_option("lml_batch", lim0)
        dev.set_option("lml_batch_mb", 1)                   # (130, 2) and up: not two scratch sets in a MiB
        dev.timing_reset()
        rows_equal(dev.loo_objective_batch(r["T"], True), r["single"])
        assert dev.timing("loo_traces")[1] == 5
    finally:
        dev.set_option("lml_batch", lim0)
        dev.set_option("lml_batch_mb", mb0)


# ------------------------------------------------------------------------------------ 8. the fit
def make_gpr(n_restarts=3):
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as C, WhiteKernel
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    b = np.array([[0.0, 1.0], [0.0, 1.0]])
    kernel = C(1.0, [1e-3, 1e4]) * RBF([1.0, 1.0], [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    return GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=n_restarts, noise_level=1e-2,
                                    preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                    account_for_inf=None, random_state=7)


def fit_data(n):
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (n, 2))
    return X, np.sin(3 * X.sum(1)) + 0.2 * rng.standard_normal(n)


@pytest.mark.parametrize("n,n_restarts", [(120, 3), (300, 8)])
def test_side_by_side_loo_fit_is_the_sequential_fit(n, n_restarts, monkeypatch):
    from gpry_amd import lockstep
    if n_restarts >= 8:
        # up to 300 points ``batch_contexts`` deals the runs to one group: two, so that a second context takes part
        monkeypatch.setenv("GPRY_HIP_FIT_BATCH_CONTEXTS", "2")
    X, y = fit_data(n)
    seq = make_gpr(n_restarts).append_to_data(X, y, fit_gpr={"objective": "loo"})
    assert seq.fit_stats["objective"] == "loo" and seq.fit_stats["side_by_side"] is False and seq.fit_stats["why"]
    forms = [make_gpr(n_restarts).append_to_data(X, y, fit_gpr={"objective": "loo", "side_by_side": True})]
    g = make_gpr(n_restarts)
    g.fit_loo_side_by_side = True
    forms.append(g.append_to_data(X, y, fit_gpr={"objective": "loo"}))
    g = make_gpr(n_restarts).append_to_data(X, y, fit_gpr=False)
    forms.append(g.fit_gpr_hyperparameters(objective="loo", side_by_side=True))
    for g in forms:
        st = g.fit_stats
        if lockstep.available():
            print(f"side by side: {st['contexts']} context(s), evaluations per run {st['evals_per_run']}")
            assert st["side_by_side"] is True and st["why"] == "" and st["schedule"] == "latency"
        else:
            print(f"no lock-step driver for this scipy: the fit fell back ({st['why']})")
            assert st["side_by_side"] is False and st["why"] == lockstep.why()
        assert st["objective"] == "loo"
        assert np.array_equal(g.kernel_.theta, seq.kernel_.theta)
        assert g.loo_value_ == seq.loo_value_
        assert g.log_marginal_likelihood_value_ == seq.log_marginal_likelihood_value_
    if lockstep.available() and n_restarts >= 8:
        assert all(g.fit_stats["contexts"] > 1 for g in forms)          # more than one group context took part
    with pytest.raises(ValueError, match="side_by_side"):
        forms[0].fit_gpr_hyperparameters(objective="lml", side_by_side=True)
